// Sim3Solver (src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (src/LoopClosing.cc:284-345), as functions of one thread:
// the staging of a pair, the draw of three pairs, Horn's closed form from two 3x3 float matrices (psl_ss_hypothesis), the inlier test
// of a pair, the iteration budget, and the driver psl_ss_iterate in the reference's order.  Product code.  Plain C++ text: the kernel
// (pslfe_sim3_solver.hip) includes it for the device and tools/dropin/sim3_solver_main.cpp for its host loop (define
// PSL_SIM3_SOLVER_HOST_ONLY there to build without the library), so both run the same single IEEE operations (build with
// -ffp-contract=off).  The kernel shares everything but the driver: it evaluates a block of hypotheses at once and takes the first
// that qualifies (its header says why that is the same result).  tests/sim3_solver_cases.py is the same text in numpy.
// Restated from the reference, rounding by rounding (DESIGN.md §3 lists every convention):
//   the thresholds, FromCameraToImage          src/Sim3Solver.cc:84-88, :405-423; include/Sim3Solver.h:78-79 (vector<size_t>)
//   SetRansacParameters                        :114-138
//   the draw                                   :163-177: psl_rs_draw<3> of ransac_kernels.h, with glibc's rand() and RandomInt
//   ComputeCentroid, ComputeSim3               :215-337
//   Project, CheckInliers                      :382-403, :340-364
//   iterate                                    :140-207
// OpenCV is not in the reference tree: where the solver hands a step to it (reduce, Mat products, eigen, norm, Rodrigues, the
// MatExpr scales and gemm folds) the order written here is this library's reading of OpenCV 3.2; parity with OpenCV is unpinned.
// sin / cos are psl_glibc_sin / psl_glibc_cos; atan2 is psl_atan2 (fdlibm's, at most one ulp off glibc's: psl_f64math.h).
#ifndef PSL_SIM3_SOLVER_KERNELS_H
#define PSL_SIM3_SOLVER_KERNELS_H

#include "pose_kernels.h"   // psl_glibc_sin, psl_glibc_cos
#include "ransac_kernels.h"

#ifndef PSL_F64_QUAL
#define PSL_F64_QUAL PSL_PO_HD
#endif
#include "psl_f64math.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define PSL_SS_HD PSL_PO_HD
#define PSL_SS_STAGED_FLOATS 12     // X1[3] X2[3] p1[2] p2[2] th1 th2
#define PSL_SS_SINCOS_RANGE 105414350.0   // psl_sincos_glibc.h

struct PslSsCams {
    float fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
};

// One hypothesis: what ComputeSim3 leaves in mR12i, mt12i, ms12i, mT12i (rows 0..2: sR | t) and mT21i (sRinv | tinv)
struct PslSsHyp {
    float R[9], t[3], s;
    float T12[12], T21[12];   // row-major 3x4
};

// ---- the iteration budget (SetRansacParameters :114-138): host arithmetic with the host's libm, tabulated per N for the device -----
#include <math.h>
static inline int psl_ss_max_iterations(double prob, int min_inliers, int max_its, int N) {
    int n;
    if (N == min_inliers) n = 1;
    else {
        const float epsilon = (float)min_inliers / (float)N;
        const double v = ceil(log(1 - prob) / log(1 - pow((double)epsilon, 3)));
        n = v < (double)max_its ? (int)v : max_its;   // min(nIterations, maxIts) taken before the conversion: an infinite ratio is maxIts
    }
    if (n > max_its) n = max_its;
    return n < 1 ? 1 : n;
}

// ---- staging (the constructor :84-109) ------------------------------------------------------------------------------------------------
// mvnMaxError is a vector<size_t>: 9.210 * sigma2 is a double product truncated to an unsigned integer, and the test compares a float
// with that integer converted to float.
PSL_SS_HD float psl_ss_max_error(float sigma2) {
    const double v = 9.210 * (double)sigma2;
    if (!(v >= 0.0)) return 0.f;                          // the host conversion would be undefined
    if (v >= 9223372036854775808.0) return 9223372036854775808.f;
    return (float)(unsigned long long)v;
}
// FromCameraToImage (:405-423): invz = 1 / z in float; fx * x + cx is two float operations
PSL_SS_HD void psl_ss_to_image(const float* X, float fx, float fy, float cx, float cy, float* p) {
    const float invz = PSL_RS_FDIV(1.f, X[2]);
    const float x = X[0] * invz, y = X[1] * invz;
    p[0] = fx * x + cx;
    p[1] = fy * y + cy;
}
// row: a PslSim3Pair (12 floats: u1 v1 is1 u2 v2 is2 P1c[3] P2c[3]); sig: mvLevelSigma2 of the two keypoints' octaves
PSL_SS_HD void psl_ss_stage(const float* row, const float* sig, const PslSsCams* K, float* o) {
    for (int r = 0; r < 3; ++r) { o[r] = row[6 + r]; o[3 + r] = row[9 + r]; }
    psl_ss_to_image(o, K->fx1, K->fy1, K->cx1, K->cy1, o + 6);
    psl_ss_to_image(o + 3, K->fx2, K->fy2, K->cx2, K->cy2, o + 8);
    o[10] = psl_ss_max_error(sig[0]);
    o[11] = psl_ss_max_error(sig[1]);
}

// ---- ComputeSim3 (:226-337) --------------------------------------------------------------------------------------------------------
// ComputeCentroid (:215-224).  P is 3x3 row-major, column i = point i.  cv::reduce(P, C, 1, SUM) on CV_32F: (p0 + p2) + p1, the two
// accumulators of reduceC_ for three columns; C / P.cols: C * (float)(1.0 / 3.0); Pr.col(i) = P.col(i) - C in float.
PSL_SS_HD void psl_ss_centroid(const float* P, float* Pr, float* C) {
    const float third = (float)(1.0 / 3.0);
    for (int r = 0; r < 3; ++r) {
        C[r] = ((P[3 * r] + P[3 * r + 2]) + P[3 * r + 1]) * third;
        for (int i = 0; i < 3; ++i) Pr[3 * r + i] = P[3 * r + i] - C[r];
    }
}

// the templated hypot above OpenCV's JacobiImpl_, in double
PSL_SS_HD double psl_ss_hypot(double a, double b) {
    a = __builtin_fabs(a);
    b = __builtin_fabs(b);
    if (a > b) { b = PSL_PO_DIV(b, a); return a * PSL_PO_SQRT(1.0 + b * b); }
    if (b > 0) { a = PSL_PO_DIV(a, b); return b * PSL_PO_SQRT(1.0 + a * a); }
    return 0.0;
}

// the pivot bookkeeping of JacobiImpl_: the column of the largest |A[k][m]|, m > k, and the row of the largest |A[i][k]|, i < k
PSL_SS_HD int psl_ss_jacobi_ind_r(const float* A, int k) {
    int m = k + 1;
    float mv = __builtin_fabsf(A[4 * k + m]);
    for (int i = k + 2; i < 4; ++i) {
        const float v = __builtin_fabsf(A[4 * k + i]);
        if (mv < v) { mv = v; m = i; }
    }
    return m;
}
PSL_SS_HD int psl_ss_jacobi_ind_c(const float* A, int k) {
    int m = 0;
    float mv = __builtin_fabsf(A[k]);
    for (int i = 1; i < k; ++i) {
        const float v = __builtin_fabsf(A[4 * i + k]);
        if (mv < v) { mv = v; m = i; }
    }
    return m;
}

#define PSL_SS_ROTATE(v0, v1)                            \
    do {                                                 \
        const float a0_ = (v0), b0_ = (v1);              \
        (v0) = a0_ * c - b0_ * s;                        \
        (v1) = a0_ * s + b0_ * c;                        \
    } while (0)

// cv::eigen on a symmetric 4x4 CV_32F: the cyclic Jacobi of OpenCV 3.2 (JacobiImpl_<float>) with its indR / indC pivot bookkeeping;
// the rotation (hypot, t, c, s) is computed in double and applied in float; at most n*n*30 rotations; then a selection sort by
// decreasing eigenvalue.  A (upper triangle read and destroyed), W the eigenvalues, V the eigenvectors as ROWS, with the sign the
// rotations leave.  Returns the rotations made.
PSL_SS_HD int psl_ss_jacobi4(float* A, float* W, float* V) {
    const int n = 4;
    int indR[4] = {0, 0, 0, 0}, indC[4] = {0, 0, 0, 0};
    for (int i = 0; i < 16; ++i) V[i] = (i % 5) == 0 ? 1.f : 0.f;
    for (int k = 0; k < n; ++k) {
        W[k] = A[5 * k];
        if (k < n - 1) indR[k] = psl_ss_jacobi_ind_r(A, k);
        if (k > 0) indC[k] = psl_ss_jacobi_ind_c(A, k);
    }
    int iters = 0;
    for (; iters < n * n * 30; ++iters) {
        int k = 0;
        float mv = __builtin_fabsf(A[indR[0]]);
        for (int i = 1; i < n - 1; ++i) {
            const float v = __builtin_fabsf(A[4 * i + indR[i]]);
            if (mv < v) { mv = v; k = i; }
        }
        int l = indR[k];
        for (int i = 1; i < n; ++i) {
            const float v = __builtin_fabsf(A[4 * indC[i] + i]);
            if (mv < v) { mv = v; k = indC[i]; l = i; }
        }
        const float p = A[4 * k + l];
        if (!(__builtin_fabsf(p) > PSL_RS_FLT_EPSILON)) break;   // also ends on a NaN pivot (the reference would spin to its limit)
        const double pd = (double)p, y = (double)(W[l] - W[k]) * 0.5;
        double td = __builtin_fabs(y) + psl_ss_hypot(pd, y);
        double sd = psl_ss_hypot(pd, td);
        const double cd = PSL_PO_DIV(td, sd);
        sd = PSL_PO_DIV(pd, sd);
        td = PSL_PO_DIV(pd, td) * pd;
        if (y < 0) { sd = -sd; td = -td; }
        const float c = (float)cd, s = (float)sd, t = (float)td;
        A[4 * k + l] = 0.f;
        W[k] = W[k] - t;
        W[l] = W[l] + t;
        for (int i = 0; i < k; ++i) PSL_SS_ROTATE(A[4 * i + k], A[4 * i + l]);
        for (int i = k + 1; i < l; ++i) PSL_SS_ROTATE(A[4 * k + i], A[4 * i + l]);
        for (int i = l + 1; i < n; ++i) PSL_SS_ROTATE(A[4 * k + i], A[4 * l + i]);
        for (int i = 0; i < n; ++i) PSL_SS_ROTATE(V[4 * k + i], V[4 * l + i]);
        for (int j = 0; j < 2; ++j) {
            const int idx = j == 0 ? k : l;
            if (idx < n - 1) indR[idx] = psl_ss_jacobi_ind_r(A, idx);
            if (idx > 0) indC[idx] = psl_ss_jacobi_ind_c(A, idx);
        }
    }
    for (int k = 0; k < n - 1; ++k) {
        int m = k;
        for (int i = k + 1; i < n; ++i)
            if (W[m] < W[i]) m = i;
        if (k != m) {
            const float w = W[m]; W[m] = W[k]; W[k] = w;
            for (int i = 0; i < n; ++i) { const float v = V[4 * m + i]; V[4 * m + i] = V[4 * k + i]; V[4 * k + i] = v; }
        }
    }
    return iters;
}

// cv::Rodrigues on a float 1x3: widened to double; theta = sqrt(x^2 + y^2 + z^2) in index order; theta < DBL_EPSILON: identity;
// else c, s from the restated glibc cos / sin, c1 = 1 - c, r *= 1 / theta, R_ij = (c I_ij + c1 rr^T_ij) + s [r]x_ij in double, rounded
// to float.  A theta outside the range of the restated sin / cos (a NaN: the degenerate quaternion (1, 0, 0, 0) gives 0 / 0) gives NaN
// in every entry, which is what glibc's sin / cos of a NaN give.
PSL_SS_HD void psl_ss_rodrigues(const float* v, const double* tab, float* R) {
    double r[3] = {(double)v[0], (double)v[1], (double)v[2]};
    const double theta = PSL_PO_SQRT((r[0] * r[0] + r[1] * r[1]) + r[2] * r[2]);
    if (theta < PSL_RS_DBL_EPSILON) {
        for (int i = 0; i < 9; ++i) R[i] = (i % 4) == 0 ? 1.f : 0.f;
        return;
    }
    if (!(theta < PSL_SS_SINCOS_RANGE)) {
        for (int i = 0; i < 9; ++i) R[i] = __builtin_nanf("");
        return;
    }
    const double c = psl_glibc_cos(theta, tab), s = psl_glibc_sin(theta, tab), c1 = 1.0 - c;
    const double it = PSL_PO_DIV(1.0, theta);
    r[0] = r[0] * it; r[1] = r[1] * it; r[2] = r[2] * it;
    const double rx[9] = {0.0, -r[2], r[1], r[2], 0.0, -r[0], -r[1], r[0], 0.0};
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) R[3 * i + j] = (float)((c * (i == j ? 1.0 : 0.0) + c1 * (r[i] * r[j])) + s * rx[3 * i + j]);
}

// one row of a float 3x3 * 3x1 product: the double sum in index order of the exact double products
PSL_SS_HD double psl_ss_row3(const float* M, const float* X) {
    return ((double)M[0] * (double)X[0] + (double)M[1] * (double)X[1]) + (double)M[2] * (double)X[2];
}

// P1, P2: 3x3 row-major, column i = the camera coordinates of drawn pair i in KF1 / KF2
PSL_SS_HD void psl_ss_hypothesis(const float* P1, const float* P2, int fix_scale, const double* tab, PslSsHyp* H) {
    float Pr1[9], Pr2[9], O1[3], O2[3];
    psl_ss_centroid(P1, Pr1, O1);
    psl_ss_centroid(P2, Pr2, O2);
    // M = Pr2 * Pr1.t() (:243): per element the double sum in index order, rounded once
    float M[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[3 * i + j] = (float)psl_ss_row3(Pr2 + 3 * i, Pr1 + 3 * j);
    // N (:251-265): the operands are floats, so C++ forms each sum in float, left to right, before widening it to the double N11..N44;
    // Mat_<float> << then stores that float unchanged
    const float N11 = (M[0] + M[4]) + M[8], N12 = M[5] - M[7], N13 = M[6] - M[2], N14 = M[1] - M[3];
    const float N22 = (M[0] - M[4]) - M[8], N23 = M[1] + M[3], N24 = M[6] + M[2];
    const float N33 = (-M[0] + M[4]) - M[8], N34 = M[5] + M[7], N44 = (-M[0] - M[4]) + M[8];
    float A[16] = {N11, N12, N13, N14, N12, N22, N23, N24, N13, N23, N33, N34, N14, N24, N34, N44};
    float W[4], V[16];
    psl_ss_jacobi4(A, W, V);
    // vec = evec.row(0).colRange(1, 4); ang = atan2(norm(vec), evec(0, 0)); vec = 2 * ang * vec / norm(vec) (:274-280)
    const double nrm = PSL_PO_SQRT(((double)V[1] * (double)V[1] + (double)V[2] * (double)V[2]) + (double)V[3] * (double)V[3]);
    const double ang = psl_atan2(nrm, (double)V[0]);
    const float alpha = (float)PSL_PO_DIV(2.0 * ang, nrm);
    const float vec[3] = {V[1] * alpha, V[2] * alpha, V[3] * alpha};
    psl_ss_rodrigues(vec, tab, H->R);
    const float* R = H->R;
    if (!fix_scale) {   // :292-309
        float P3[9];
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 3; ++j) {
                const float col[3] = {Pr2[j], Pr2[3 + j], Pr2[6 + j]};
                P3[3 * i + j] = (float)psl_ss_row3(R + 3 * i, col);
            }
        double nom = 0.0, den = 0.0;
        for (int i = 0; i < 9; ++i) nom = nom + (double)Pr1[i] * (double)P3[i];
        for (int i = 0; i < 9; ++i) den = den + (double)(P3[i] * P3[i]);   // cv::pow(P3, 2): the float square
        H->s = (float)PSL_PO_DIV(nom, den);
    } else {
        H->s = 1.0f;
    }
    const float s = H->s;
    // mt12i = O1 - ms12i * mR12i * O2 (:316): one gemm(R, O2, -s, O1, 1)
    for (int r = 0; r < 3; ++r) H->t[r] = (float)(psl_ss_row3(R + 3 * r, O2) * (double)(-s) + (double)O1[r]);
    // sR = s * R; sRinv = (1.0 / s) * R.t(); tinv = -sRinv * t (:323-336)
    const float is = (float)PSL_PO_DIV(1.0, (double)s);
    float sRinv[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            H->T12[4 * i + j] = s * R[3 * i + j];
            sRinv[3 * i + j] = is * R[3 * j + i];
            H->T21[4 * i + j] = sRinv[3 * i + j];
        }
    for (int r = 0; r < 3; ++r) {
        H->T12[4 * r + 3] = H->t[r];
        H->T21[4 * r + 3] = (float)(-psl_ss_row3(sRinv + 3 * r, H->t));
    }
}

// ---- Project and CheckInliers for one pair (:382-403, :340-364) ---------------------------------------------------------------------
// Rcw * X + tcw under the convention above PslPose (the double sum plus the translation, rounded once); invz = 1 / z in float.  A point
// behind the camera is not guarded; a NaN error is "not an inlier" by the <.
PSL_SS_HD void psl_ss_project(const float* T, const float* X, float fx, float fy, float cx, float cy, float* p) {
    float Pc[3];
    for (int r = 0; r < 3; ++r) Pc[r] = (float)(psl_ss_row3(T + 4 * r, X) + (double)T[4 * r + 3]);
    psl_ss_to_image(Pc, fx, fy, cx, cy, p);
}
// dist.dot(dist) on a 2x1 CV_32F: the double sum of the two exact squares, rounded to the float err
PSL_SS_HD float psl_ss_err(const float* a, const float* b) {
    const float d0 = a[0] - b[0], d1 = a[1] - b[1];
    return (float)((double)d0 * (double)d0 + (double)d1 * (double)d1);
}
// q: a staged pair
PSL_SS_HD int psl_ss_inlier(const float* q, const PslSsHyp* H, const PslSsCams* K) {
    float p2im1[2], p1im2[2];
    psl_ss_project(H->T12, q + 3, K->fx1, K->fy1, K->cx1, K->cy1, p2im1);
    psl_ss_project(H->T21, q, K->fx2, K->fy2, K->cx2, K->cy2, p1im2);
    const float err1 = psl_ss_err(q + 6, p2im1), err2 = psl_ss_err(p1im2, q + 8);
    return (err1 < q[10] && err2 < q[11]) ? 1 : 0;
}

PSL_SS_HD void psl_ss_gather(const float* q0, const float* q1, const float* q2, float* P1, float* P2) {
    const float* q[3] = {q0, q1, q2};
    for (int i = 0; i < 3; ++i)
        for (int r = 0; r < 3; ++r) { P1[3 * r + i] = q[i][r]; P2[3 * r + i] = q[i][3 + r]; }
}

// ---- iterate (:140-207) on one core ---------------------------------------------------------------------------------------------------
// staged [N][12]; max_its = psl_ss_max_iterations(.., N); the candidate's stream is srand(seed) at iteration 0 and three draws per
// iteration, so a call that starts at iteration start_it skips 3 * start_it draws.  flags [N] (by pair row) is written in full.
// status / iterations / ninliers / best / H as PslSim3SolverResult (include/pslfe.h); H is written only with status 1.
// trace (may be NULL, else room for n_iterations entries): the draw, the hypothesis and the count of every iteration the call ran.
struct PslSsOutcome {
    int status, iterations, ninliers, best;
};
struct PslSsTrace {
    int32_t idx[3], cnt;
    PslSsHyp h;
};
PSL_SS_HD PslSsOutcome psl_ss_iterate(const float* staged, int N, const PslSsCams* K, int max_its, int min_inliers, int fix_scale, uint32_t seed,
                                      int start_it, int best_in, int n_iterations, const double* tab, PslSsHyp* H, uint8_t* flags,
                                      PslSsTrace* trace) {
    PslSsOutcome o = {0, start_it, 0, best_in};
    for (int i = 0; i < N; ++i) flags[i] = 0;
    if (N < min_inliers) { o.status = 2; return o; }
    PslRsRand G;
    if (start_it < max_its && n_iterations > 0) {   // a call that runs no iteration draws nothing
        psl_rs_srand(&G, seed);
        for (int i = 0; i < 3 * start_it; ++i) psl_rs_rand(&G);
    }
    int cur = 0;
    while (o.iterations < max_its && cur < n_iterations) {
        ++cur;
        ++o.iterations;
        int idx[3];
        psl_rs_draw<3>(&G, N, idx);
        float P1[9], P2[9];
        psl_ss_gather(staged + 12 * idx[0], staged + 12 * idx[1], staged + 12 * idx[2], P1, P2);
        PslSsHyp h;
        psl_ss_hypothesis(P1, P2, fix_scale, tab, &h);
        int cnt = 0;
        for (int i = 0; i < N; ++i) cnt += psl_ss_inlier(staged + 12 * i, &h, K);
        if (trace) {
            PslSsTrace* t = trace + (cur - 1);
            t->idx[0] = idx[0]; t->idx[1] = idx[1]; t->idx[2] = idx[2]; t->cnt = cnt;
            t->h = h;
        }
        if (cnt >= o.best) {
            o.best = cnt;
            if (cnt > min_inliers) {
                o.status = 1;
                o.ninliers = cnt;
                *H = h;
                for (int i = 0; i < N; ++i) flags[i] = (uint8_t)psl_ss_inlier(staged + 12 * i, &h, K);
                return o;
            }
        }
    }
    if (o.iterations >= max_its) o.status = 2;
    return o;
}

#endif
