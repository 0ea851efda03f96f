// psl-slam_amd/csrc/ransac_kernels.h alone on the host, for tests/test_ransac_shared_cpu.py.  Reads cases from the file argv[1] and
// prints one line of hexadecimal bit patterns per case:
//   draw K N seed its                 its draws of psl_rs_draw<K> (K = 3, 4, 8) on one stream of srand(seed): its * K indices
//   svd f|d ES m n want_v eps         psl_rs_jacobi_svd<float|double, ES> (ES = 1, 4) on n rows of length m; eps as the bits of a double.
//     <n * m words> x ES              one line per interleaved workspace; every workspace is solved, the first is printed:
//                                     a (n * m), w (n doubles), v (n * n, with want_v)
// Build: g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined tests/ransac_host.cpp
#include <inttypes.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../psl-slam_amd/csrc/ransac_kernels.h"

template <typename T>
static T from_bits(uint64_t u) {
    T x;
    if (sizeof(T) == 4) { const uint32_t h = (uint32_t)u; memcpy(&x, &h, 4); }
    else memcpy(&x, &u, 8);
    return x;
}
template <typename T>
static void print_bits(T x) {
    if (sizeof(T) == 4) { uint32_t h; memcpy(&h, &x, 4); printf(" %" PRIx32, h); }
    else { uint64_t u; memcpy(&u, &x, 8); printf(" %" PRIx64, u); }
}
static uint64_t word(FILE* f) {
    uint64_t u = 0;
    if (fscanf(f, "%" SCNx64, &u) != 1) { fprintf(stderr, "short case file\n"); exit(2); }
    return u;
}

template <int K>
static void draws(int N, uint32_t seed, int its) {
    PslRsRand G;
    psl_rs_srand(&G, seed);
    for (int it = 0; it < its; ++it) {
        int idx[K];
        psl_rs_draw<K>(&G, N, idx);
        for (int k = 0; k < K; ++k) printf(" %x", (unsigned)idx[k]);
    }
}

template <typename T, int ES>
static void svd(FILE* f, int m, int n, int want_v, double eps) {
    std::vector<T> a((size_t)n * m * ES), v((size_t)n * n * ES);
    std::vector<double> w((size_t)n * ES);
    for (int s = 0; s < ES; ++s)
        for (int k = 0; k < n * m; ++k) a[(size_t)k * ES + s] = from_bits<T>(word(f));
    for (int s = 0; s < ES; ++s) psl_rs_jacobi_svd<T, ES>(a.data() + s, m, n, w.data() + s, want_v ? v.data() + s : (T*)nullptr, eps);
    for (int k = 0; k < n * m; ++k) print_bits(a[(size_t)k * ES]);
    for (int k = 0; k < n; ++k) print_bits(w[(size_t)k * ES]);
    for (int k = 0; want_v && k < n * n; ++k) print_bits(v[(size_t)k * ES]);
}

int main(int argc, char** argv) {
    FILE* f = argc == 2 ? fopen(argv[1], "r") : nullptr;
    if (!f) { fprintf(stderr, "usage: ransac_host <cases.txt>\n"); return 2; }
    char what[8], type[8];
    while (fscanf(f, "%7s", what) == 1) {
        if (!strcmp(what, "draw")) {
            int K, N, its;
            unsigned seed;
            if (fscanf(f, "%d %d %u %d", &K, &N, &seed, &its) != 4 || N < K) return 2;
            if (K == 3) draws<3>(N, seed, its);
            else if (K == 4) draws<4>(N, seed, its);
            else if (K == 8) draws<8>(N, seed, its);
            else return 2;
        } else if (!strcmp(what, "svd")) {
            int ES, m, n, want_v;
            if (fscanf(f, "%7s %d %d %d %d", type, &ES, &m, &n, &want_v) != 5 || m < 1 || n < 1 || (ES != 1 && ES != 4)) return 2;
            const double eps = from_bits<double>(word(f));
            if (type[0] == 'f') { if (ES == 1) svd<float, 1>(f, m, n, want_v, eps); else svd<float, 4>(f, m, n, want_v, eps); }
            else { if (ES == 1) svd<double, 1>(f, m, n, want_v, eps); else svd<double, 4>(f, m, n, want_v, eps); }
        } else {
            return 2;
        }
        printf("\n");
    }
    fclose(f);
    return 0;
}
