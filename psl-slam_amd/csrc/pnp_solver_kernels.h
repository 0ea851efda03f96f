// PnPsolver (src/PnPsolver.cc), the EPnP RANSAC of Tracking::Relocalization (src/Tracking.cc:2075-2101), as functions of one thread:
// the staging of a row, the draw of four rows, compute_pose (EPnP in double) in stages, the inlier test of a row, the iteration
// budget, and the driver psl_pnp_iterate in the reference's order.  Product code.  Plain C++ text: the kernel (pslfe_pnp.hip) includes it
// for the device and tools/dropin/pnp_main.cpp for its host loop (define PSL_PNP_HOST_ONLY there to build without the library), so both
// run the same single IEEE operations (build with -ffp-contract=off).  tests/pnp_cases.py is the same text in numpy.
// Restated from the reference, rounding by rounding (DESIGN.md §3 lists every convention):
//   the constructor's staging                  src/PnPsolver.cc:67-110; include/PnPsolver.h:128 (double fu, fv, uc, vc)
//   SetRansacParameters                        :121-157
//   the draw                                   :188-201; Thirdparty/DBoW2/DUtils/Random.cpp:47-50
//   iterate, Refine, CheckInliers              :165-258, :260-305, :308-339
//   compute_pose and everything under it       :375-950
// glibc's rand(), RandomInt and the draw (psl_rs_draw<4>) are those of ransac_kernels.h: included, not copied.
// OpenCV is not in the reference tree: where the solver hands a step to it (cvMulTransposed, cvSVD, cvInvert, cvSolve) the order
// written here is this library's reading of OpenCV 3.2; parity with OpenCV is unpinned.
//   cvMulTransposed(A, dst, 1)   A^T A: every upper-triangle entry the sequential sum over the rows of A in row order, from 0.0; the
//                                lower triangle is copied.
//   cvSVD                        psl_pnp_jacobi: JacobiSVDImpl_<double> as ransac_kernels.h reads it, with eps = 10 * DBL_EPSILON, then
//                                the rows normalised by 1 / w (0 where w <= DBL_MIN): oracle/glue_oracle.cpp:70-138 at any n.
//                                After it the rows of At are the left singular vectors (U^T) and the rows of Vt the right ones (V^T).
//                                CV_SVD_U_T hands out U^T = At (:400, :493 read its rows); without a flag U[i][k] = At[k][i] and
//                                V[j][k] = Vt[k][j] (:608-612: R = U V^T).
//   cvInvert(.., CV_SVD)         that SVD plus back-substitution on the identity: x[r][c] = sum_i Vt[i][r] * (At[i][c] * (1 / w_i)), i
//                                ascending from 0.0, the directions with w_i <= 2 * DBL_EPSILON * sum(w) left out (a planar point set
//                                gives a pseudo-inverse).
//   cvSolve(.., CV_SVD)          that SVD of the 6 x n matrix plus back-substitution on one right-hand side: s = (sum_j At[i][j] *
//                                b[j]) * (1 / w_i); x[j] = x[j] + s * Vt[i][j], the same threshold.
// One thing the reference leaves open: qr_solve returns early on eta == 0 and leaves X as it was, and gauss_newton's x[4] is not
// initialised; here x starts at 0.0 in every gauss_newton.
#ifndef PSL_PNP_SOLVER_KERNELS_H
#define PSL_PNP_SOLVER_KERNELS_H

#include <math.h>   // the iteration budget

#include "ransac_kernels.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

// every function is inlined into its caller: a call on the device would put a frame into scratch memory
#define PSL_PNP_HD __attribute__((always_inline)) PSL_PO_HD
#define PSL_PNP_MIN_SET 4
#define PSL_PNP_DBL_MIN 2.2250738585072014e-308
#define PSL_PNP_ROW_FLOATS 7   // u v X Y Z sigma2*th2 (mvMaxError) and one spare word: an odd stride in LDS

// The workspace of one compute_pose, in doubles.  Element k of a workspace lies at ws[k * ES]: ES = 1 on the host; the kernel
// interleaves the workspaces of a block of hypotheses (ES = the block) so that the lanes of a wave touch consecutive doubles.
enum {
    PSL_PNP_AT = 0,      // 144  MtM, then Ut (the 12x12 Jacobi works in place)
    PSL_PNP_D = 144,     // 12
    PSL_PNP_L = 156,     // 60   l_6x10
    PSL_PNP_RHO = 216,   // 6
    PSL_PNP_CWS = 222,   // 12   cws[4][3]
    PSL_PNP_CCS = 234,   // 12   ccs[4][3]
    PSL_PNP_SA = 246,    // 36   the small SVDs' At (n rows of m <= 6); gauss_newton's a[24] and b[6]
    PSL_PNP_SV = 282,    // 25   their Vt; gauss_newton's x[4], A1[4], A2[4]
    PSL_PNP_SW = 307,    // 5    their w
    PSL_PNP_M3 = 312,    // 9    pw0tpw0, then cc, then abt
    PSL_PNP_CI = 321,    // 9    cc_inv
    PSL_PNP_BET = 330,   // 4    the betas of the current trial
    PSL_PNP_RT = 334,    // 12   R (9) and t (3) of the current trial
    PSL_PNP_RTB = 346,   // 12   of the best trial so far
    PSL_PNP_PC0 = 358,   // 3
    PSL_PNP_PW0 = 361,   // 3
    PSL_PNP_SGN = 364,   // 1    1.0 when solve_for_sign negated ccs and pcs
    PSL_PNP_ERR = 365,   // 2    the reprojection error of the current trial and of the best
    PSL_PNP_B5 = 367,    // 5    the solution of cvSolve
    PSL_PNP_WS = 372
};
#define PSL_PNP_GA PSL_PNP_SA
#define PSL_PNP_GB (PSL_PNP_SA + 24)
#define PSL_PNP_GX PSL_PNP_SV
#define PSL_PNP_G1 (PSL_PNP_SV + 4)
#define PSL_PNP_G2 (PSL_PNP_SV + 8)
#define W_(k) ws[(size_t)(k) * ES]

struct PslPnpCam {
    double fu, fv, uc, vc;   // widened from the frame's floats
};

// Where the staged rows are: the first lds_n in `lds` (stride PSL_PNP_ROW_FLOATS), the others staged from their PslPnpRow (6 floats)
// where they are used.  The host keeps lds_n = 0.
struct PslPnpRows {
    const float* lds;
    int lds_n;
    const float* rows;
    float th2;
};
// staging (:87-93, :154-156): mvMaxError = sigma2 * th2, a float product
PSL_PNP_HD void psl_pnp_stage(const float* row, float th2, float* o) {
    o[0] = row[0]; o[1] = row[1]; o[2] = row[2]; o[3] = row[3]; o[4] = row[4];
    o[5] = row[5] * th2;
}
PSL_PNP_HD void psl_pnp_load(const PslPnpRows* R, int i, float* q) {
    if (i < R->lds_n) {
        for (int k = 0; k < 6; ++k) q[k] = R->lds[PSL_PNP_ROW_FLOATS * (size_t)i + k];
    } else {
        psl_pnp_stage(R->rows + 6 * (size_t)i, R->th2, q);
    }
}

// The correspondences of one compute_pose: the four drawn rows (idx, span 4) or the rows whose flag is set, ascending (Refine :262-281)
struct PslPnpSel {
    const int* idx;
    const uint8_t* flags;
    int span;   // 4, or the row count
    int n;      // number_of_correspondences
};
PSL_PNP_HD double psl_pnp_pick3(const double* v, int k) { return k == 0 ? v[0] : (k == 1 ? v[1] : v[2]); }
PSL_PNP_HD int psl_pnp_sel_row(const PslPnpSel* S, int k) {
    if (S->idx) return S->idx[k];
    return S->flags[k] ? k : -1;
}
// add_correspondence (:363-373): the floats widened
PSL_PNP_HD void psl_pnp_corr(const PslPnpRows* R, int i, double* pw, double* us) {
    float q[6];
    psl_pnp_load(R, i, q);
    us[0] = (double)q[0]; us[1] = (double)q[1];
    pw[0] = (double)q[2]; pw[1] = (double)q[3]; pw[2] = (double)q[4];
}

// ---- the iteration budget (SetRansacParameters :121-152): host arithmetic with the host's libm, tabulated per N for the device -----
// Returns mRansacMaxIts; *min_out = mRansacMinInliers after the two clamps.  nIterations is a double before its conversion to int: a
// NaN (epsilon above 1, only with N < minInliers, where iterate leaves at once), an infinite or a negative ratio (1 - epsilon^3 rounds
// to 1 beyond N of 8e5) would be undefined in the conversion and count as max_its here.
static inline int psl_pnp_max_iterations(double prob, int min_inliers, int max_its, int min_set, float epsilon, int N, int* min_out) {
    int nMin = (int)((float)N * epsilon);
    if (nMin < min_inliers) nMin = min_inliers;
    if (nMin < min_set) nMin = min_set;
    *min_out = nMin;
    if (N < 1) return 1;
    float eps = epsilon;
    if (eps < (float)nMin / (float)N) eps = (float)nMin / (float)N;
    int n;
    if (nMin == N) n = 1;
    else {
        const double v = ceil(log(1 - prob) / log(1 - pow((double)eps, 3)));
        n = (v == v && v > -1.0 && v < (double)max_its) ? (int)v : max_its;
    }
    if (n > max_its) n = max_its;
    return n < 1 ? 1 : n;
}

// ---- cvSVD: the sweeps and the sort of psl_rs_jacobi_svd<double> word for word (both are held to tests/pnp_cases.py) on the n rows of
// length m at ws[a..], w at ws[w..], Vt at ws[v..] (v < 0: none), then the rows divided by their singular value.  Written on offsets:
// through the template's pointers k_pnp_solve runs 0.2 to 0.5 % longer at 12288 candidates (profiles/ransac_shared_ab.json) ---------
template <int ES>
PSL_PNP_HD void psl_pnp_jacobi(double* ws, int a, int m, int n, int w, int v) {
    const double eps = PSL_RS_DBL_EPSILON * 10;
    const int max_iter = m > 30 ? m : 30;
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) { const double t = W_(a + i * m + k); sd = sd + t * t; }
        W_(w + i) = sd;
        if (v >= 0)
            for (int k = 0; k < n; ++k) W_(v + i * n + k) = k == i ? 1.0 : 0.0;
    }
    for (int iter = 0; iter < max_iter; ++iter) {
        bool changed = false;
        for (int i = 0; i < n - 1; ++i)
            for (int j = i + 1; j < n; ++j) {
                double aa = W_(w + i), p = 0, bb = W_(w + j);
                for (int k = 0; k < m; ++k) p = p + W_(a + i * m + k) * W_(a + j * m + k);
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
                    const double x = W_(a + i * m + k), y = W_(a + j * m + k);
                    const double t0 = c * x + s * y, t1 = -s * x + c * y;
                    W_(a + i * m + k) = t0; W_(a + j * m + k) = t1;
                    aa = aa + t0 * t0; bb = bb + t1 * t1;
                }
                W_(w + i) = aa; W_(w + j) = bb;
                changed = true;
                if (v >= 0)
                    for (int k = 0; k < n; ++k) {
                        const double x = W_(v + i * n + k), y = W_(v + j * n + k);
                        W_(v + i * n + k) = c * x + s * y;
                        W_(v + j * n + k) = -s * x + c * y;
                    }
            }
        if (!changed) break;
    }
    for (int i = 0; i < n; ++i) {
        double sd = 0;
        for (int k = 0; k < m; ++k) { const double t = W_(a + i * m + k); sd = sd + t * t; }
        W_(w + i) = PSL_PO_SQRT(sd);
    }
    for (int i = 0; i < n - 1; ++i) {
        int j = i;
        for (int k = i + 1; k < n; ++k)
            if (W_(w + j) < W_(w + k)) j = k;
        if (i != j) {
            { const double t = W_(w + i); W_(w + i) = W_(w + j); W_(w + j) = t; }
            for (int k = 0; k < m; ++k) { const double t = W_(a + i * m + k); W_(a + i * m + k) = W_(a + j * m + k); W_(a + j * m + k) = t; }
            if (v >= 0)
                for (int k = 0; k < n; ++k) { const double t = W_(v + i * n + k); W_(v + i * n + k) = W_(v + j * n + k); W_(v + j * n + k) = t; }
        }
    }
    for (int i = 0; i < n; ++i) {
        const double wi = W_(w + i);
        const double s = wi > PSL_PNP_DBL_MIN ? PSL_PO_DIV(1.0, wi) : 0.;
        for (int k = 0; k < m; ++k) W_(a + i * m + k) = W_(a + i * m + k) * s;
    }
}
// the threshold of SVBkSb: 2 * DBL_EPSILON * (w_0 + w_1 + ...)
template <int ES>
PSL_PNP_HD double psl_pnp_bksb_threshold(const double* ws, int w, int n) {
    double t = 0;
    for (int i = 0; i < n; ++i) t = t + W_(w + i);
    return t * (PSL_RS_DBL_EPSILON * 2);
}

// ---- choose_control_points (:375-409) in three steps: two sets of sums over the correspondences, then the PCA -------------------------
// cws[0][j], before the division
template <int ES>
PSL_PNP_HD double psl_pnp_sum_cw0(const PslPnpRows* R, const PslPnpSel* S, int j) {
    double s = 0;
    for (int k = 0; k < S->span; ++k) {
        const int i = psl_pnp_sel_row(S, k);
        if (i < 0) continue;
        double pw[3], us[2];
        psl_pnp_corr(R, i, pw, us);
        s = s + psl_pnp_pick3(pw, j);
    }
    return s;
}
// entry e = 0..5 of the upper triangle of PW0^T PW0: (0,0) (0,1) (0,2) (1,1) (1,2) (2,2); cws[0] is final
template <int ES>
PSL_PNP_HD double psl_pnp_sum_pwpw(const double* ws, const PslPnpRows* R, const PslPnpSel* S, int e) {
    const int a = e < 3 ? 0 : (e < 5 ? 1 : 2), b = e < 3 ? e : (e < 5 ? e - 2 : 2);
    const double ca = W_(PSL_PNP_CWS + a), cb = W_(PSL_PNP_CWS + b);
    double s = 0;
    for (int k = 0; k < S->span; ++k) {
        const int i = psl_pnp_sel_row(S, k);
        if (i < 0) continue;
        double pw[3], us[2];
        psl_pnp_corr(R, i, pw, us);
        s = s + (psl_pnp_pick3(pw, a) - ca) * (psl_pnp_pick3(pw, b) - cb);
    }
    return s;
}
PSL_PNP_HD void psl_pnp_tri3(int e, int* a, int* b) {
    *a = e < 3 ? 0 : (e < 5 ? 1 : 2);
    *b = e < 3 ? e : (e < 5 ? e - 2 : 2);
}
// M3 holds PW0^T PW0 (full).  cvSVD(U_T): dc, uct; cws[1..3]; then compute_barycentric_coordinates' cc and cc_inv (:411-421)
template <int ES>
PSL_PNP_HD void psl_pnp_control_points(double* ws, int ncorr) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W_(PSL_PNP_SA + 3 * i + j) = W_(PSL_PNP_M3 + 3 * j + i);
    psl_pnp_jacobi<ES>(ws, PSL_PNP_SA, 3, 3, PSL_PNP_SW, -1);
    for (int i = 1; i < 4; ++i) {
        const double k = PSL_PO_SQRT(PSL_PO_DIV(W_(PSL_PNP_SW + i - 1), (double)ncorr));
        for (int j = 0; j < 3; ++j) W_(PSL_PNP_CWS + 3 * i + j) = W_(PSL_PNP_CWS + j) + k * W_(PSL_PNP_SA + 3 * (i - 1) + j);
    }
    for (int i = 0; i < 3; ++i)
        for (int j = 1; j < 4; ++j) W_(PSL_PNP_M3 + 3 * i + j - 1) = W_(PSL_PNP_CWS + 3 * j + i) - W_(PSL_PNP_CWS + i);
    // cvInvert(CC, CC_inv, CV_SVD)
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W_(PSL_PNP_SA + 3 * i + j) = W_(PSL_PNP_M3 + 3 * j + i);
    psl_pnp_jacobi<ES>(ws, PSL_PNP_SA, 3, 3, PSL_PNP_SW, PSL_PNP_SV);
    const double thr = psl_pnp_bksb_threshold<ES>(ws, PSL_PNP_SW, 3);
    for (int k = 0; k < 9; ++k) W_(PSL_PNP_CI + k) = 0.0;
    for (int i = 0; i < 3; ++i) {
        const double w = W_(PSL_PNP_SW + i);
        if (__builtin_fabs(w) <= thr) continue;
        const double wi = PSL_PO_DIV(1.0, w);
        for (int r = 0; r < 3; ++r)
            for (int c = 0; c < 3; ++c)
                W_(PSL_PNP_CI + 3 * r + c) = W_(PSL_PNP_CI + 3 * r + c) + W_(PSL_PNP_SV + 3 * i + r) * (W_(PSL_PNP_SA + 3 * i + c) * wi);
    }
}
// the alphas of one correspondence (:423-433)
template <int ES>
PSL_PNP_HD void psl_pnp_alphas(const double* ws, const double* pw, double* a) {
    const double d0 = pw[0] - W_(PSL_PNP_CWS), d1 = pw[1] - W_(PSL_PNP_CWS + 1), d2 = pw[2] - W_(PSL_PNP_CWS + 2);
    for (int j = 0; j < 3; ++j) a[1 + j] = (W_(PSL_PNP_CI + 3 * j) * d0 + W_(PSL_PNP_CI + 3 * j + 1) * d1) + W_(PSL_PNP_CI + 3 * j + 2) * d2;
    a[0] = ((1.0 - a[1]) - a[2]) - a[3];
}
// element (row r = 0 / 1 of the pair of rows, column c) of fill_M (:436-451)
PSL_PNP_HD double psl_pnp_m(const double* a, const double* us, const PslPnpCam* K, int r, int c) {
    const int j = c / 3;
    const double as = j == 0 ? a[0] : (j == 1 ? a[1] : (j == 2 ? a[2] : a[3]));
    const int k = c % 3;
    if (r == 0) return k == 0 ? as * K->fu : (k == 1 ? 0.0 : as * (K->uc - us[0]));
    return k == 0 ? 0.0 : (k == 1 ? as * K->fv : as * (K->vc - us[1]));
}
// entry e = 0..77 of the upper triangle of M^T M (row p, column q >= p, row by row): the sum over the 2 n rows of M in row order
PSL_PNP_HD void psl_pnp_tri12(int e, int* p, int* q) {
    int r = 0;
    while (e >= 12 - r) { e -= 12 - r; ++r; }
    *p = r; *q = r + e;
}
template <int ES>
PSL_PNP_HD double psl_pnp_sum_mtm(const double* ws, const PslPnpRows* R, const PslPnpSel* S, const PslPnpCam* K, int p, int q) {
    double s = 0;
    for (int k = 0; k < S->span; ++k) {
        const int i = psl_pnp_sel_row(S, k);
        if (i < 0) continue;
        double pw[3], us[2], a[4];
        psl_pnp_corr(R, i, pw, us);
        psl_pnp_alphas<ES>(ws, pw, a);
        s = s + psl_pnp_m(a, us, K, 0, p) * psl_pnp_m(a, us, K, 0, q);
        s = s + psl_pnp_m(a, us, K, 1, p) * psl_pnp_m(a, us, K, 1, q);
    }
    return s;
}

PSL_PNP_HD double psl_pnp_dot3(double a0, double a1, double a2, double b0, double b1, double b2) { return (a0 * b0 + a1 * b1) + a2 * b2; }

// AT holds M^T M (full).  cvSVD(U_T) in place; compute_L_6x10 (:760-800); compute_rho (:802-810)
template <int ES>
PSL_PNP_HD void psl_pnp_null_space(double* ws) {
    psl_pnp_jacobi<ES>(ws, PSL_PNP_AT, 12, 12, PSL_PNP_D, -1);
    for (int i = 0; i < 6; ++i) {
        // pair i of (a, b): (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
        const int a = i < 3 ? 0 : (i < 5 ? 1 : 2), b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
        double dv[4][3];
        for (int v = 0; v < 4; ++v)
            for (int k = 0; k < 3; ++k) dv[v][k] = W_(PSL_PNP_AT + 12 * (11 - v) + 3 * a + k) - W_(PSL_PNP_AT + 12 * (11 - v) + 3 * b + k);
#define PSL_PNP_DD(x, y) psl_pnp_dot3(dv[x][0], dv[x][1], dv[x][2], dv[y][0], dv[y][1], dv[y][2])
        W_(PSL_PNP_L + 10 * i + 0) = PSL_PNP_DD(0, 0);
        W_(PSL_PNP_L + 10 * i + 1) = 2.0 * PSL_PNP_DD(0, 1);
        W_(PSL_PNP_L + 10 * i + 2) = PSL_PNP_DD(1, 1);
        W_(PSL_PNP_L + 10 * i + 3) = 2.0 * PSL_PNP_DD(0, 2);
        W_(PSL_PNP_L + 10 * i + 4) = 2.0 * PSL_PNP_DD(1, 2);
        W_(PSL_PNP_L + 10 * i + 5) = PSL_PNP_DD(2, 2);
        W_(PSL_PNP_L + 10 * i + 6) = 2.0 * PSL_PNP_DD(0, 3);
        W_(PSL_PNP_L + 10 * i + 7) = 2.0 * PSL_PNP_DD(1, 3);
        W_(PSL_PNP_L + 10 * i + 8) = 2.0 * PSL_PNP_DD(2, 3);
        W_(PSL_PNP_L + 10 * i + 9) = PSL_PNP_DD(3, 3);
#undef PSL_PNP_DD
        // dist2(cws[a], cws[b])
        const double e0 = W_(PSL_PNP_CWS + 3 * a) - W_(PSL_PNP_CWS + 3 * b), e1 = W_(PSL_PNP_CWS + 3 * a + 1) - W_(PSL_PNP_CWS + 3 * b + 1),
                     e2 = W_(PSL_PNP_CWS + 3 * a + 2) - W_(PSL_PNP_CWS + 3 * b + 2);
        W_(PSL_PNP_RHO + i) = (e0 * e0 + e1 * e1) + e2 * e2;
    }
}

// cvSolve(L_6xn, Rho, B, CV_SVD) with the columns col[0..n) of l_6x10; the solution is left in B5
template <int ES>
PSL_PNP_HD void psl_pnp_solve6(double* ws, int n, const int* col) {
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < 6; ++j) W_(PSL_PNP_SA + 6 * i + j) = W_(PSL_PNP_L + 10 * j + col[i]);
    psl_pnp_jacobi<ES>(ws, PSL_PNP_SA, 6, n, PSL_PNP_SW, PSL_PNP_SV);
    const double thr = psl_pnp_bksb_threshold<ES>(ws, PSL_PNP_SW, n);
    for (int j = 0; j < n; ++j) W_(PSL_PNP_B5 + j) = 0.0;
    for (int i = 0; i < n; ++i) {
        const double w = W_(PSL_PNP_SW + i);
        if (__builtin_fabs(w) <= thr) continue;
        const double wi = PSL_PO_DIV(1.0, w);
        double s = 0;
        for (int j = 0; j < 6; ++j) s = s + W_(PSL_PNP_SA + 6 * i + j) * W_(PSL_PNP_RHO + j);
        s = s * wi;
        for (int j = 0; j < n; ++j) W_(PSL_PNP_B5 + j) = W_(PSL_PNP_B5 + j) + s * W_(PSL_PNP_SV + n * i + j);
    }
}

// find_betas_approx_1 / _2 / _3 (:667-758) into BET
template <int ES>
PSL_PNP_HD void psl_pnp_betas_approx(double* ws, int which) {
    double b[4], t0, t1, t2 = 0.0, t3 = 0.0;
    if (which == 1) {
        const int col[4] = {0, 1, 3, 6};
        psl_pnp_solve6<ES>(ws, 4, col);
        for (int j = 0; j < 4; ++j) b[j] = W_(PSL_PNP_B5 + j);
        if (b[0] < 0) {
            t0 = PSL_PO_SQRT(-b[0]);
            t1 = PSL_PO_DIV(-b[1], t0); t2 = PSL_PO_DIV(-b[2], t0); t3 = PSL_PO_DIV(-b[3], t0);
        } else {
            t0 = PSL_PO_SQRT(b[0]);
            t1 = PSL_PO_DIV(b[1], t0); t2 = PSL_PO_DIV(b[2], t0); t3 = PSL_PO_DIV(b[3], t0);
        }
    } else {
        const int col[5] = {0, 1, 2, 3, 4};
        psl_pnp_solve6<ES>(ws, which == 2 ? 3 : 5, col);
        for (int j = 0; j < 4; ++j) b[j] = W_(PSL_PNP_B5 + j);
        if (b[0] < 0) {
            t0 = PSL_PO_SQRT(-b[0]);
            t1 = (b[2] < 0) ? PSL_PO_SQRT(-b[2]) : 0.0;
        } else {
            t0 = PSL_PO_SQRT(b[0]);
            t1 = (b[2] > 0) ? PSL_PO_SQRT(b[2]) : 0.0;
        }
        if (b[1] < 0) t0 = -t0;
        if (which == 3) t2 = PSL_PO_DIV(b[3], t0);
    }
    W_(PSL_PNP_BET) = t0; W_(PSL_PNP_BET + 1) = t1; W_(PSL_PNP_BET + 2) = t2; W_(PSL_PNP_BET + 3) = t3;
}

// qr_solve (:860-950) on gauss_newton's 6x4 a, b, x, in its operation order: the search for eta never looks at the last row, and a
// zero eta returns with x as it was
template <int ES>
PSL_PNP_HD void psl_pnp_qr_solve(double* ws) {
    const int nr = 6, nc = 4;
#define A_(i, j) W_(PSL_PNP_GA + (i) * nc + (j))
    for (int k = 0; k < nc; ++k) {
        double eta = __builtin_fabs(A_(k, k));
        for (int i = k + 1; i < nr; ++i) {
            const double elt = __builtin_fabs(A_(i - 1, k));
            if (eta < elt) eta = elt;
        }
        if (eta == 0) {
            W_(PSL_PNP_G1 + k) = 0.0; W_(PSL_PNP_G2 + k) = 0.0;
            return;
        }
        double sum = 0.0;
        const double inv_eta = PSL_PO_DIV(1., eta);
        for (int i = k; i < nr; ++i) {
            const double t = A_(i, k) * inv_eta;
            A_(i, k) = t;
            sum = sum + t * t;
        }
        double sigma = PSL_PO_SQRT(sum);
        if (A_(k, k) < 0) sigma = -sigma;
        A_(k, k) = A_(k, k) + sigma;
        const double a1 = sigma * A_(k, k);
        W_(PSL_PNP_G1 + k) = a1;
        W_(PSL_PNP_G2 + k) = -eta * sigma;
        for (int j = k + 1; j < nc; ++j) {
            double s = 0;
            for (int i = k; i < nr; ++i) s = s + A_(i, k) * A_(i, j);
            const double tau = PSL_PO_DIV(s, a1);
            for (int i = k; i < nr; ++i) A_(i, j) = A_(i, j) - tau * A_(i, k);
        }
    }
    for (int j = 0; j < nc; ++j) {   // b <- Qt b
        double tau = 0;
        for (int i = j; i < nr; ++i) tau = tau + A_(i, j) * W_(PSL_PNP_GB + i);
        tau = PSL_PO_DIV(tau, W_(PSL_PNP_G1 + j));
        for (int i = j; i < nr; ++i) W_(PSL_PNP_GB + i) = W_(PSL_PNP_GB + i) - tau * A_(i, j);
    }
    W_(PSL_PNP_GX + nc - 1) = PSL_PO_DIV(W_(PSL_PNP_GB + nc - 1), W_(PSL_PNP_G2 + nc - 1));   // X = R-1 b
    for (int i = nc - 2; i >= 0; --i) {
        double s = 0;
        for (int j = i + 1; j < nc; ++j) s = s + A_(i, j) * W_(PSL_PNP_GX + j);
        W_(PSL_PNP_GX + i) = PSL_PO_DIV(W_(PSL_PNP_GB + i) - s, W_(PSL_PNP_G2 + i));
    }
#undef A_
}

// gauss_newton (:840-858) with compute_A_and_b_gauss_newton (:812-838) on BET
template <int ES>
PSL_PNP_HD void psl_pnp_gauss_newton(double* ws) {
    for (int k = 0; k < 4; ++k) W_(PSL_PNP_GX + k) = 0.0;
    for (int it = 0; it < 5; ++it) {
        const double b0 = W_(PSL_PNP_BET), b1 = W_(PSL_PNP_BET + 1), b2 = W_(PSL_PNP_BET + 2), b3 = W_(PSL_PNP_BET + 3);
        for (int i = 0; i < 6; ++i) {
            double l[10];
            for (int k = 0; k < 10; ++k) l[k] = W_(PSL_PNP_L + 10 * i + k);
            W_(PSL_PNP_GA + 4 * i + 0) = (((2 * l[0]) * b0 + l[1] * b1) + l[3] * b2) + l[6] * b3;
            W_(PSL_PNP_GA + 4 * i + 1) = ((l[1] * b0 + (2 * l[2]) * b1) + l[4] * b2) + l[7] * b3;
            W_(PSL_PNP_GA + 4 * i + 2) = ((l[3] * b0 + l[4] * b1) + (2 * l[5]) * b2) + l[8] * b3;
            W_(PSL_PNP_GA + 4 * i + 3) = ((l[6] * b0 + l[7] * b1) + l[8] * b2) + (2 * l[9]) * b3;
            W_(PSL_PNP_GB + i) = W_(PSL_PNP_RHO + i) -
                                 ((((((((((l[0] * b0) * b0 + (l[1] * b0) * b1) + (l[2] * b1) * b1) + (l[3] * b0) * b2) + (l[4] * b1) * b2) +
                                      (l[5] * b2) * b2) + (l[6] * b0) * b3) + (l[7] * b1) * b3) + (l[8] * b2) * b3) + (l[9] * b3) * b3);
        }
        psl_pnp_qr_solve<ES>(ws);
        for (int i = 0; i < 4; ++i) W_(PSL_PNP_BET + i) = W_(PSL_PNP_BET + i) + W_(PSL_PNP_GX + i);
    }
}

// compute_ccs (:453-464) from BET
template <int ES>
PSL_PNP_HD void psl_pnp_ccs(double* ws) {
    for (int k = 0; k < 12; ++k) W_(PSL_PNP_CCS + k) = 0.0;
    for (int i = 0; i < 4; ++i)
        for (int k = 0; k < 12; ++k) W_(PSL_PNP_CCS + k) = W_(PSL_PNP_CCS + k) + W_(PSL_PNP_BET + i) * W_(PSL_PNP_AT + 12 * (11 - i) + k);
}
// compute_pcs (:466-475) of one correspondence, with the sign of solve_for_sign (:636-649) applied to the result: ccs keeps its sign
// here, and the negation of every term is the negation of the rounded sum
template <int ES>
PSL_PNP_HD void psl_pnp_pc(const double* ws, const double* pw, int negate, double* pc) {
    double a[4];
    psl_pnp_alphas<ES>(ws, pw, a);
    for (int j = 0; j < 3; ++j) {
        const double v = ((a[0] * W_(PSL_PNP_CCS + j) + a[1] * W_(PSL_PNP_CCS + 3 + j)) + a[2] * W_(PSL_PNP_CCS + 6 + j)) + a[3] * W_(PSL_PNP_CCS + 9 + j);
        pc[j] = negate ? -v : v;
    }
}
// solve_for_sign: pcs[2] of the first correspondence alone
template <int ES>
PSL_PNP_HD void psl_pnp_sign(double* ws, const PslPnpRows* R, const PslPnpSel* S) {
    double sgn = 0.0;
    for (int k = 0; k < S->span; ++k) {
        const int i = psl_pnp_sel_row(S, k);
        if (i < 0) continue;
        double pw[3], us[2], pc[3];
        psl_pnp_corr(R, i, pw, us);
        psl_pnp_pc<ES>(ws, pw, 0, pc);
        if (pc[2] < 0.0) sgn = 1.0;
        break;
    }
    W_(PSL_PNP_SGN) = sgn;
}
// estimate_R_and_t (:569-627).  e = 0..2: pc0[e]; 3..5: pw0[e - 3], before the division
template <int ES>
PSL_PNP_HD double psl_pnp_sum_c0(const double* ws, const PslPnpRows* R, const PslPnpSel* S, int e) {
    const int neg = W_(PSL_PNP_SGN) != 0.0;
    double s = 0;
    for (int k = 0; k < S->span; ++k) {
        const int i = psl_pnp_sel_row(S, k);
        if (i < 0) continue;
        double pw[3], us[2], pc[3];
        psl_pnp_corr(R, i, pw, us);
        if (e < 3) { psl_pnp_pc<ES>(ws, pw, neg, pc); s = s + psl_pnp_pick3(pc, e); }
        else s = s + psl_pnp_pick3(pw, e - 3);
    }
    return s;
}
// abt[3 * j + c], e = 3 * j + c; PC0 and PW0 are final
template <int ES>
PSL_PNP_HD double psl_pnp_sum_abt(const double* ws, const PslPnpRows* R, const PslPnpSel* S, int e) {
    const int neg = W_(PSL_PNP_SGN) != 0.0, j = e / 3, c = e % 3;
    const double pcj = W_(PSL_PNP_PC0 + j), pwc = W_(PSL_PNP_PW0 + c);
    double s = 0;
    for (int k = 0; k < S->span; ++k) {
        const int i = psl_pnp_sel_row(S, k);
        if (i < 0) continue;
        double pw[3], us[2], pc[3];
        psl_pnp_corr(R, i, pw, us);
        psl_pnp_pc<ES>(ws, pw, neg, pc);
        s = s + (psl_pnp_pick3(pc, j) - pcj) * (psl_pnp_pick3(pw, c) - pwc);
    }
    return s;
}
// M3 holds abt.  cvSVD(ABt, D, U, V): R = U V^T, the det < 0 flip of row 2, t into RT
template <int ES>
PSL_PNP_HD void psl_pnp_rt(double* ws) {
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) W_(PSL_PNP_SA + 3 * i + j) = W_(PSL_PNP_M3 + 3 * j + i);
    psl_pnp_jacobi<ES>(ws, PSL_PNP_SA, 3, 3, PSL_PNP_SW, PSL_PNP_SV);
    double Rm[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j)
            Rm[3 * i + j] = psl_pnp_dot3(W_(PSL_PNP_SA + i), W_(PSL_PNP_SA + 3 + i), W_(PSL_PNP_SA + 6 + i), W_(PSL_PNP_SV + j), W_(PSL_PNP_SV + 3 + j),
                                         W_(PSL_PNP_SV + 6 + j));
    const double det = (((((Rm[0] * Rm[4]) * Rm[8] + (Rm[1] * Rm[5]) * Rm[6]) + (Rm[2] * Rm[3]) * Rm[7]) - (Rm[2] * Rm[4]) * Rm[6]) -
                        (Rm[1] * Rm[3]) * Rm[8]) - (Rm[0] * Rm[5]) * Rm[7];
    if (det < 0) { Rm[6] = -Rm[6]; Rm[7] = -Rm[7]; Rm[8] = -Rm[8]; }
    for (int k = 0; k < 9; ++k) W_(PSL_PNP_RT + k) = Rm[k];
    const double w0 = W_(PSL_PNP_PW0), w1 = W_(PSL_PNP_PW0 + 1), w2 = W_(PSL_PNP_PW0 + 2);
    for (int i = 0; i < 3; ++i) W_(PSL_PNP_RT + 9 + i) = W_(PSL_PNP_PC0 + i) - psl_pnp_dot3(Rm[3 * i], Rm[3 * i + 1], Rm[3 * i + 2], w0, w1, w2);
}
// reprojection_error (:550-567), before the division
template <int ES>
PSL_PNP_HD double psl_pnp_sum_reproj(const double* ws, const PslPnpRows* R, const PslPnpSel* S, const PslPnpCam* K) {
    double Rt[12];
    for (int k = 0; k < 12; ++k) Rt[k] = W_(PSL_PNP_RT + k);
    double sum2 = 0.0;
    for (int k = 0; k < S->span; ++k) {
        const int i = psl_pnp_sel_row(S, k);
        if (i < 0) continue;
        double pw[3], us[2];
        psl_pnp_corr(R, i, pw, us);
        const double Xc = psl_pnp_dot3(Rt[0], Rt[1], Rt[2], pw[0], pw[1], pw[2]) + Rt[9];
        const double Yc = psl_pnp_dot3(Rt[3], Rt[4], Rt[5], pw[0], pw[1], pw[2]) + Rt[10];
        const double inv_Zc = PSL_PO_DIV(1.0, psl_pnp_dot3(Rt[6], Rt[7], Rt[8], pw[0], pw[1], pw[2]) + Rt[11]);
        const double ue = K->uc + (K->fu * Xc) * inv_Zc, ve = K->vc + (K->fv * Yc) * inv_Zc;
        sum2 = sum2 + PSL_PO_SQRT((us[0] - ue) * (us[0] - ue) + (us[1] - ve) * (us[1] - ve));
    }
    return sum2;
}
// the choice of N by < in the order 1, 2, 3 (:518-522): trial `which` has its R, t in RT and its error in ERR
template <int ES>
PSL_PNP_HD void psl_pnp_keep(double* ws, int which) {
    if (which == 1 || W_(PSL_PNP_ERR) < W_(PSL_PNP_ERR + 1)) {
        for (int k = 0; k < 12; ++k) W_(PSL_PNP_RTB + k) = W_(PSL_PNP_RT + k);
        W_(PSL_PNP_ERR + 1) = W_(PSL_PNP_ERR);
    }
}

// compute_pose (:477-525) on one thread; R, t are left in RTB
template <int ES>
PSL_PNP_HD void psl_pnp_compute_pose(double* ws, const PslPnpRows* R, const PslPnpSel* S, const PslPnpCam* K) {
    const double dn = (double)S->n;
    for (int j = 0; j < 3; ++j) W_(PSL_PNP_CWS + j) = PSL_PO_DIV(psl_pnp_sum_cw0<ES>(R, S, j), dn);
    for (int e = 0; e < 6; ++e) {
        int a, b;
        psl_pnp_tri3(e, &a, &b);
        const double v = psl_pnp_sum_pwpw<ES>(ws, R, S, e);
        W_(PSL_PNP_M3 + 3 * a + b) = v; W_(PSL_PNP_M3 + 3 * b + a) = v;
    }
    psl_pnp_control_points<ES>(ws, S->n);
    for (int e = 0; e < 78; ++e) {
        int p, q;
        psl_pnp_tri12(e, &p, &q);
        const double v = psl_pnp_sum_mtm<ES>(ws, R, S, K, p, q);
        W_(PSL_PNP_AT + 12 * p + q) = v; W_(PSL_PNP_AT + 12 * q + p) = v;
    }
    psl_pnp_null_space<ES>(ws);
    for (int which = 1; which <= 3; ++which) {
        psl_pnp_betas_approx<ES>(ws, which);
        psl_pnp_gauss_newton<ES>(ws);
        psl_pnp_ccs<ES>(ws);
        psl_pnp_sign<ES>(ws, R, S);
        for (int e = 0; e < 6; ++e) W_(PSL_PNP_PC0 + e) = PSL_PO_DIV(psl_pnp_sum_c0<ES>(ws, R, S, e), dn);
        for (int e = 0; e < 9; ++e) W_(PSL_PNP_M3 + e) = psl_pnp_sum_abt<ES>(ws, R, S, e);
        psl_pnp_rt<ES>(ws);
        W_(PSL_PNP_ERR) = PSL_PO_DIV(psl_pnp_sum_reproj<ES>(ws, R, S, K), dn);
        psl_pnp_keep<ES>(ws, which);
    }
}

// ---- CheckInliers for one row (:314-337), with its mixed widths: Xc, Yc and invZc are floats, ue and ve doubles, the distances and
// error2 floats.  A point behind the camera is not guarded; a NaN error is "not an inlier" by the <.  Rt: R (9) and t (3) in double
PSL_PNP_HD int psl_pnp_inlier(const float* q, const double* Rt, const PslPnpCam* K) {
    const double x = (double)q[2], y = (double)q[3], z = (double)q[4];
    const float Xc = (float)(((Rt[0] * x + Rt[1] * y) + Rt[2] * z) + Rt[9]);
    const float Yc = (float)(((Rt[3] * x + Rt[4] * y) + Rt[5] * z) + Rt[10]);
    const float invZc = (float)PSL_PO_DIV(1.0, ((Rt[6] * x + Rt[7] * y) + Rt[8] * z) + Rt[11]);
    const double ue = K->uc + (K->fu * (double)Xc) * (double)invZc;
    const double ve = K->vc + (K->fv * (double)Yc) * (double)invZc;
    const float distX = (float)((double)q[0] - ue), distY = (float)((double)q[1] - ve);
    const float error2 = distX * distX + distY * distY;
    return error2 < q[5] ? 1 : 0;
}

// ---- iterate (:165-258) with Refine (:260-305) on one core ----------------------------------------------------------------------------
// rows [N] PslPnpRow; max_its / min_inliers = psl_pnp_max_iterations(.., N, ..).  The candidate's stream is srand(seed) at iteration 0
// and four draws per iteration, so a call that starts at iteration `iterations` skips 4 * iterations draws.  The solver's state is
// (iterations, best, best_T, best_flags [N] = mvbBestInliers), read and written.  The loop is the reference's: it runs while
// mnIterations < mRansacMaxIts OR the call has run fewer than n_iterations, i.e. max(max_its - iterations, n_iterations) iterations
// unless a Refine succeeds.  status: bit 0 = a pose was returned (T, ninliers, flags [N] hold it), bit 1 = bNoMore.  flags is written in
// full.  ws: PSL_PNP_WS doubles.
struct PslPnpOutcome {
    int status, iterations, ninliers, best;
};
PSL_PNP_HD void psl_pnp_to_float(const double* Rt, float* T) {
    for (int k = 0; k < 12; ++k) T[k] = (float)Rt[k];
}
PSL_PNP_HD PslPnpOutcome psl_pnp_iterate(const float* rows, int N, const PslPnpCam* K, float th2, int max_its, int min_inliers, uint32_t seed,
                                        int iterations, int best_in, float* best_T, uint8_t* best_flags, int n_iterations, double* ws,
                                        float* T, uint8_t* flags) {
    PslPnpOutcome o = {0, iterations, 0, best_in};
    for (int i = 0; i < N; ++i) flags[i] = 0;
    for (int k = 0; k < 12; ++k) T[k] = 0.f;
    if (N < min_inliers) { o.status = 2; return o; }
    PslPnpRows R = {nullptr, 0, rows, th2};
    PslRsRand G;
    if (o.iterations < max_its || n_iterations > 0) {   // a call that runs no iteration draws nothing
        psl_rs_srand(&G, seed);
        for (int i = 0; i < 4 * iterations; ++i) psl_rs_rand(&G);
    }
    int cur = 0;
    while (o.iterations < max_its || cur < n_iterations) {
        ++cur;
        ++o.iterations;
        int idx[4];
        psl_rs_draw<4>(&G, N, idx);
        PslPnpSel S = {idx, nullptr, 4, 4};
        psl_pnp_compute_pose<1>(ws, &R, &S, K);
        double Rt[12];
        for (int k = 0; k < 12; ++k) Rt[k] = ws[PSL_PNP_RTB + k];
        int cnt = 0;
        for (int i = 0; i < N; ++i) {
            float q[6];
            psl_pnp_load(&R, i, q);
            flags[i] = (uint8_t)psl_pnp_inlier(q, Rt, K);
            cnt += flags[i];
        }
        if (cnt >= min_inliers) {
            if (cnt > o.best) {
                for (int i = 0; i < N; ++i) best_flags[i] = flags[i];
                o.best = cnt;
                psl_pnp_to_float(Rt, best_T);
            }
            // Refine: on mvbBestInliers, whether or not this iteration was a new best
            int nb = 0;
            for (int i = 0; i < N; ++i) nb += best_flags[i] ? 1 : 0;
            PslPnpSel SR = {nullptr, best_flags, N, nb};
            psl_pnp_compute_pose<1>(ws, &R, &SR, K);
            for (int k = 0; k < 12; ++k) Rt[k] = ws[PSL_PNP_RTB + k];
            int rc = 0;
            for (int i = 0; i < N; ++i) {
                float q[6];
                psl_pnp_load(&R, i, q);
                flags[i] = (uint8_t)psl_pnp_inlier(q, Rt, K);
                rc += flags[i];
            }
            if (rc > min_inliers) {
                o.status = 1;
                o.ninliers = rc;
                psl_pnp_to_float(Rt, T);
                return o;
            }
        }
    }
    for (int i = 0; i < N; ++i) flags[i] = 0;
    if (o.iterations >= max_its) {
        o.status = 2;
        if (o.best >= min_inliers) {
            o.status = 3;
            o.ninliers = o.best;
            for (int i = 0; i < N; ++i) flags[i] = best_flags[i];
            for (int k = 0; k < 12; ++k) T[k] = best_T[k];
        }
    }
    return o;
}

#undef W_
#endif
