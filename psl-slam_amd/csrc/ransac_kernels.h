// What the RANSAC solvers share, as functions of one thread: glibc's rand() and DUtils::Random::RandomInt (Thirdparty/DBoW2/DUtils/
// Random.cpp:47-50), the draw of K rows without replacement (src/Sim3Solver.cc:163-177, src/PnPsolver.cc:188-201, src/Initializer.cc:
// 82-97) and this library's reading of OpenCV 3.2's one-sided Jacobi SVD (JacobiSVDImpl_; not in the reference tree, parity unpinned).
// Product code.  Plain C++ text for host and device, like the headers it serves (sim3_solver_kernels.h, pnp_solver_kernels.h,
// initializer_kernels.h): build with -ffp-contract=off.  tests/test_ransac_shared_cpu.py pins it alone on the host.  DESIGN.md §3.
// Left where they are: psl_jacobi_rows<M,N> and psl_jacobi_wave of pslfe_glue.hip, the same SVD shaped by where their data lives, on
// the gated benchmark path; psl_ss_jacobi4, an eigen Jacobi; and, because sharing them was measured and was not free (profiles/
// ransac_shared_ab.json), psl_pnp_jacobi (these sweeps on offsets into one workspace) and psl_glibc_srand of pslfe_glue.hip (this
// seeding on a ring in LDS).  A change to the reading here is made there too.
#ifndef PSL_RANSAC_KERNELS_H
#define PSL_RANSAC_KERNELS_H

#include "pose_kernels.h"   // PSL_PO_HD, PSL_PO_DIV, PSL_PO_SQRT; through lm_kernels.h PSL_LM_UNROLL

#ifdef __clang__
#pragma clang fp contract(off)
#endif

// every function is inlined into its caller: a call on the device would put a frame into scratch memory
#define PSL_RS_HD __attribute__((always_inline)) PSL_PO_HD
#if defined(__HIP_DEVICE_COMPILE__)
#define PSL_RS_FDIV(a, b) __fdiv_rn((a), (b))
#else
#define PSL_RS_FDIV(a, b) ((a) / (b))
#endif
#define PSL_RS_FLT_EPSILON 1.1920928955078125e-07f
#define PSL_RS_DBL_EPSILON 2.220446049250313e-16

// ---- glibc rand(), TYPE_3: one rand() at stream position k on a ring of 34 words; the position matters modulo 34 alone -------------
PSL_RS_HD int psl_rs_ring_rand(uint32_t* ring, int k) {
    const uint32_t v = ring[(k - 31) % 34] + ring[(k - 3) % 34];
    ring[k % 34] = v;
    return (int)(v >> 1);
}
// srand(seed): 31 words by Lehmer steps (seed 0 is seeded as 1), the first 3 again, 310 values discarded.  Returns the position.
PSL_RS_HD int psl_rs_ring_srand(uint32_t* ring, uint32_t seed) {
    int32_t prev = seed == 0 ? 1 : (int32_t)seed;
    ring[0] = (uint32_t)prev;
    for (int i = 1; i < 31; ++i) {
        const long long hi = prev / 127773, lo = prev % 127773;
        long long word = 16807 * lo - 2836 * hi;
        if (word < 0) word += 2147483647;
        prev = (int32_t)word;
        ring[i] = (uint32_t)prev;
    }
    for (int i = 31; i < 34; ++i) ring[i] = ring[i - 31];
    for (int kk = 34; kk < 34 + 310; ++kk) psl_rs_ring_rand(ring, kk);
    return 34 + 310;
}
struct PslRsRand {
    uint32_t ring[34];
    int k;
};
PSL_RS_HD void psl_rs_srand(PslRsRand* G, uint32_t seed) { G->k = psl_rs_ring_srand(G->ring, seed); }
PSL_RS_HD int psl_rs_rand(PslRsRand* G) {
    const int k = G->k;
    const int r = psl_rs_ring_rand(G->ring, k);
    G->k = k + 1 >= 34 * 64 ? k + 1 - 34 * 63 : k + 1;
    return r;
}

// DUtils::Random::RandomInt(0, d - 1): int(((double)rand() / ((double)RAND_MAX + 1.0)) * d).  rand() / 2^31 is exact and the product
// has at most 42 significant bits, so the double expression is the integer (r * d) >> 31.
PSL_RS_HD int psl_rs_random_int(int r, int d) { return (int)(((unsigned long long)(unsigned)r * (unsigned long long)(unsigned)d) >> 31); }

// K draws from 0..N-1, N >= K: an index is removed by overwriting it with the back of vAvailableIndices and popping.  The vector is never
// built: position p holds p unless an earlier removal wrote to it, and a later write wins (ascending j).  Unrolled: the slots are registers.
template <int K>
PSL_RS_HD void psl_rs_draw(PslRsRand* G, int N, int* idx) {
    int opos[K - 1], oval[K - 1];
    for (int j = 0; j < K - 1; ++j) { opos[j] = -1; oval[j] = 0; }
    int size = N;
    PSL_LM_UNROLL
    for (int i = 0; i < K; ++i) {
        const int randi = psl_rs_random_int(psl_rs_rand(G), size);
        int v = randi, back = size - 1;
        PSL_LM_UNROLL
        for (int j = 0; j < K - 1; ++j) {
            if (opos[j] == randi) v = oval[j];
            if (opos[j] == size - 1) back = oval[j];
        }
        idx[i] = v;
        if (i < K - 1) { opos[i] = randi; oval[i] = back; }
        --size;
    }
}

// ---- JacobiSVDImpl_<T> (cvSVD, cv::SVD::compute) on the n rows of length m at a (row stride m), W in w, Vt in v (n x n; nullptr:
// none).  Element k of a, w and v lies at [k * ES]: ES = 1 on the host; a kernel interleaves the workspaces of a block (ES = the block).
// One-sided Jacobi on the rows of At = A^T (with m < n the caller swaps the operands).  W starts as the squared row norms, Vt as the
// identity.  A sweep visits the pairs i < j in order and skips a pair whose dot product p has |p| <= eps * sqrt(W_i W_j); at most
// max(m, 30) sweeps, and a sweep that rotates nothing is the last.  Then W_i = the norm of row i, and a selection sort (the first of
// equal values stays first) puts W in descending order with the rows of a and v.  The rows of a stay unnormalised: 1 / w or the
// completion of a basis is the caller's.  W, p, c and s are doubles; a rotated element is the double expression rounded to T and the
// squares of the rounded elements are accumulated in double (T = double: every cast is the identity).  eps: 10 * DBL_EPSILON for
// CV_64F, 2 * FLT_EPSILON for CV_32F.
#define PSL_RS_AT(p, k) (p)[(size_t)(k) * ES]
template <typename T, int ES>
PSL_RS_HD void psl_rs_jacobi_svd(T* a, int m, int n, double* w, T* v, double eps) {
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) { const double t = (double)PSL_RS_AT(a, i * m + k); sd = sd + t * t; }
        PSL_RS_AT(w, i) = sd;
        if (v)
            for (int k = 0; k < n; ++k) PSL_RS_AT(v, i * n + k) = k == i ? (T)1 : (T)0;
    }
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                double aa = PSL_RS_AT(w, i), p = 0, bb = PSL_RS_AT(w, j);
                for (int k = 0; k < m; ++k) p = p + (double)PSL_RS_AT(a, i * m + k) * (double)PSL_RS_AT(a, j * m + k);
                if (__builtin_fabs(p) <= eps * PSL_PO_SQRT(aa * bb)) continue;
                p = p * 2;
                const double beta = aa - bb, gamma = PSL_PO_SQRT(p * p + beta * beta);
                double c, s;
                if (beta < 0) {
                    const double delta = (gamma - beta) * 0.5;
                    s = PSL_PO_SQRT(PSL_PO_DIV(delta, gamma));
                    c = PSL_PO_DIV(p, (gamma * s) * 2);
                } else {
                    c = PSL_PO_SQRT(PSL_PO_DIV(gamma + beta, gamma * 2));
                    s = PSL_PO_DIV(p, (gamma * c) * 2);
                }
                aa = bb = 0;
                for (int k = 0; k < m; ++k) {
                    const double x = (double)PSL_RS_AT(a, i * m + k), y = (double)PSL_RS_AT(a, j * m + k);
                    const T t0 = (T)(c * x + s * y), t1 = (T)(-s * x + c * y);
                    PSL_RS_AT(a, i * m + k) = t0; PSL_RS_AT(a, j * m + k) = t1;
                    aa = aa + (double)t0 * (double)t0; bb = bb + (double)t1 * (double)t1;
                }
                PSL_RS_AT(w, i) = aa; PSL_RS_AT(w, j) = bb;
                changed = true;
                if (v)
                    for (int k = 0; k < n; ++k) {
                        const double x = (double)PSL_RS_AT(v, i * n + k), y = (double)PSL_RS_AT(v, j * n + k);
                        PSL_RS_AT(v, i * n + k) = (T)(c * x + s * y);
                        PSL_RS_AT(v, j * n + k) = (T)(-s * x + c * y);
                    }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) { const double t = (double)PSL_RS_AT(a, i * m + k); sd = sd + t * t; }
        PSL_RS_AT(w, i) = PSL_PO_SQRT(sd);
    }
    for (int i = 0; i < n - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < n; ++k)
            if (PSL_RS_AT(w, j) < PSL_RS_AT(w, k)) j = k;
        if (i != j) {
            { const double t = PSL_RS_AT(w, i); PSL_RS_AT(w, i) = PSL_RS_AT(w, j); PSL_RS_AT(w, j) = t; }
            for (int k = 0; k < m; ++k) { const T t = PSL_RS_AT(a, i * m + k); PSL_RS_AT(a, i * m + k) = PSL_RS_AT(a, j * m + k); PSL_RS_AT(a, j * m + k) = t; }
            if (v)
                for (int k = 0; k < n; ++k) { const T t = PSL_RS_AT(v, i * n + k); PSL_RS_AT(v, i * n + k) = PSL_RS_AT(v, j * n + k); PSL_RS_AT(v, j * n + k) = t; }
        }
    }
}
#undef PSL_RS_AT

#endif
