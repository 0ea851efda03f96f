// The pose optimisation (pslfe_pose.hip) as functions of one thread: the per-edge arithmetic, the SE3 update and the four rounds
// psl_po_rounds, each one call of the Levenberg driver psl_lm_optimize<6> of lm_kernels.h (the iterations and trials of a round, the
// 6x6 solve, every decision g2o makes between two sums).  Product code.  Plain C++ text: the kernel includes it for the device and
// tools/dropin/pose_main.cpp for its host loop, so both run the same single IEEE operations (build with -ffp-contract=off).  The
// rounds ask their `Problem` argument for everything that is summed over the edges; the order of those sums is not here but in the
// `Problem`.  The host loop instantiates psl_po_rounds; k_pose_optimize holds the rounds and the driver's loop written out (the
// header of pslfe_pose.hip says why), so they are changed together.  Restated from the reference's g2o:
//   edge errors / Jacobians   Thirdparty/g2o/g2o/types/types_six_dof_expmap.{h,cpp} (EdgeSE3ProjectXYZOnlyPose, EdgeStereoSE3ProjectXYZOnlyPose)
//   SE3Quat, exp, product     Thirdparty/g2o/g2o/types/se3quat.h, se3_ops.hpp
//   quadratic form            Thirdparty/g2o/g2o/core/base_unary_edge.hpp
//   the rounds                src/Optimizer.cc:696-780, :1011-1022
// Eigen is not in the reference tree, so where g2o hands a step to Eigen (quaternion <-> matrix, quaternion * vector, the products
// of small matrices) the order written here is this library's: sums run in index order, left to right.  DESIGN.md §3, §5.0k.
#ifndef PSL_POSE_KERNELS_H
#define PSL_POSE_KERNELS_H

#include "lm_kernels.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define PSL_PO_HD PSL_LM_HD
#define PSL_PO_DIV(a, b) PSL_LM_DIV(a, b)
#define PSL_PO_SQRT(a) PSL_LM_SQRT(a)

#ifndef PSL_SC64_QUAL
#define PSL_SC64_QUAL PSL_PO_HD
#endif
#include "psl_sincos_glibc.h"

#define PSL_POSE_NTERMS 28   // per edge: the 21 upper-triangle values of H row by row, the 6 of b (before the sign), the robust chi2

struct PslSE3 {
    double q[4];   // x y z w
    double t[3];
};

struct PslPoseCamD {
    double fx, fy, cx, cy, bf;
};

// Huber deltas as Optimizer.cc:274-275 holds them: `const float deltaMono = sqrt(5.991)`, a double root rounded to float
#define PSL_POSE_DELTA_MONO 2.4476518630981445   /* (float)sqrt(5.991) */
#define PSL_POSE_DELTA_STEREO 2.7955322265625     /* (float)sqrt(7.815) */
#define PSL_POSE_DELTA(mono) ((mono) ? PSL_POSE_DELTA_MONO : PSL_POSE_DELTA_STEREO)   // the delta of psl_lm_huber for a point edge

PSL_PO_HD void psl_po_cross(const double* a, const double* b, double* o) {
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

// SE3Quat::normalizeRotation (se3quat.h:284-289)
PSL_PO_HD void psl_po_normalize(double* q) {
    if (q[3] < 0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
    const double n = PSL_PO_SQRT(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
    q[0] = PSL_PO_DIV(q[0], n); q[1] = PSL_PO_DIV(q[1], n); q[2] = PSL_PO_DIV(q[2], n); q[3] = PSL_PO_DIV(q[3], n);
}

// Quaterniond(R): the branch on the trace and the largest diagonal entry
PSL_PO_HD void psl_po_quat_from_R(const double* R, double* q) {
    double t = (R[0] + R[4]) + R[8];
    if (t > 0) {
        t = PSL_PO_SQRT(t + 1.0);
        q[3] = 0.5 * t;
        t = PSL_PO_DIV(0.5, t);
        q[0] = (R[7] - R[5]) * t;
        q[1] = (R[2] - R[6]) * t;
        q[2] = (R[3] - R[1]) * t;
    } else {
        int i = 0;
        if (R[4] > R[0]) i = 1;
        if (R[8] > (i ? R[4] : R[0])) i = 2;
        // i, j = (i + 1) % 3, k = (j + 1) % 3: q[i] = t / 2, w = (R(k,j) - R(j,k)) t', q[j] = (R(j,i) + R(i,j)) t', q[k] = (R(k,i) + R(i,k)) t'
        if (i == 0) {
            t = PSL_PO_SQRT(((R[0] - R[4]) - R[8]) + 1.0);
            q[0] = 0.5 * t; t = PSL_PO_DIV(0.5, t);
            q[3] = (R[7] - R[5]) * t; q[1] = (R[3] + R[1]) * t; q[2] = (R[6] + R[2]) * t;
        } else if (i == 1) {
            t = PSL_PO_SQRT(((R[4] - R[8]) - R[0]) + 1.0);
            q[1] = 0.5 * t; t = PSL_PO_DIV(0.5, t);
            q[3] = (R[2] - R[6]) * t; q[2] = (R[7] + R[5]) * t; q[0] = (R[1] + R[3]) * t;
        } else {
            t = PSL_PO_SQRT(((R[8] - R[0]) - R[4]) + 1.0);
            q[2] = 0.5 * t; t = PSL_PO_DIV(0.5, t);
            q[3] = (R[3] - R[1]) * t; q[0] = (R[2] + R[6]) * t; q[1] = (R[5] + R[7]) * t;
        }
    }
}

// Quaterniond::toRotationMatrix
PSL_PO_HD void psl_po_quat_to_R(const double* q, double* R) {
    const double tx = 2.0 * q[0], ty = 2.0 * q[1], tz = 2.0 * q[2];
    const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
    const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
    const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
    R[0] = 1.0 - (tyy + tzz); R[1] = txy - twz;         R[2] = txz + twy;
    R[3] = txy + twz;         R[4] = 1.0 - (txx + tzz); R[5] = tyz - twx;
    R[6] = txz - twy;         R[7] = tyz + twx;         R[8] = 1.0 - (txx + tyy);
}

// Quaterniond * Vector3d: uv = 2 (q.vec x v); v + w uv + q.vec x uv
PSL_PO_HD void psl_po_rotate(const double* q, const double* v, double* o) {
    double uv[3], c[3];
    psl_po_cross(q, v, uv);
    uv[0] = uv[0] + uv[0]; uv[1] = uv[1] + uv[1]; uv[2] = uv[2] + uv[2];
    psl_po_cross(q, uv, c);
    o[0] = (v[0] + q[3] * uv[0]) + c[0];
    o[1] = (v[1] + q[3] * uv[1]) + c[1];
    o[2] = (v[2] + q[3] * uv[2]) + c[2];
}

// Converter::toSE3Quat(mTcw): float -> double, SE3Quat(R, t) (se3quat.h:58-60)
PSL_PO_HD void psl_po_from_pose(const float* R9, const float* t3, PslSE3* T) {
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = (double)R9[i];
    psl_po_quat_from_R(R, T->q);
    psl_po_normalize(T->q);
    for (int i = 0; i < 3; ++i) T->t[i] = (double)t3[i];
}

// Converter::toCvMat(SE3Quat): to_homogeneous_matrix, double -> float
PSL_PO_HD void psl_po_to_pose(const PslSE3* T, float* R9, float* t3) {
    double R[9];
    psl_po_quat_to_R(T->q, R);
    for (int i = 0; i < 9; ++i) R9[i] = (float)R[i];
    for (int i = 0; i < 3; ++i) t3[i] = (float)T->t[i];
}

// a 3x3 product, every entry (a0 b0 + a1 b1) + a2 b2
PSL_PO_HD void psl_po_mat3mul(const double* A, const double* B, double* C) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) C[3 * i + k] = (A[3 * i] * B[k] + A[3 * i + 1] * B[3 + k]) + A[3 * i + 2] * B[6 + k];
}

// SE3Quat::exp (se3quat.h:227-261): x = (omega, upsilon); tab: the table of psl_sincos_glibc.h
PSL_PO_HD void psl_po_exp(const double* x, PslSE3* T, const double* tab) {
    const double theta = PSL_PO_SQRT((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const double O[9] = {0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0};
    double O2[9], R[9], V[9];
    psl_po_mat3mul(O, O, O2);
    if (theta < 0.00001) {
        for (int i = 0; i < 9; ++i) {
            R[i] = (((i % 4) == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
            V[i] = R[i];
        }
    } else {
        const double s = psl_glibc_sin(theta, tab), c = psl_glibc_cos(theta, tab);
        const double th2 = theta * theta;
        const double a = PSL_PO_DIV(s, theta), b = PSL_PO_DIV(1.0 - c, th2), g = PSL_PO_DIV(theta - s, th2 * theta);
        for (int i = 0; i < 9; ++i) {
            const double I = (i % 4) == 0 ? 1.0 : 0.0;
            R[i] = (I + a * O[i]) + b * O2[i];
            V[i] = (I + b * O[i]) + g * O2[i];
        }
    }
    psl_po_quat_from_R(R, T->q);
    psl_po_normalize(T->q);
    for (int i = 0; i < 3; ++i) T->t[i] = (V[3 * i] * x[3] + V[3 * i + 1] * x[4]) + V[3 * i + 2] * x[5];
}

// SE3Quat::operator* (se3quat.h:104-110): A * B
PSL_PO_HD void psl_po_mul(const PslSE3* A, const PslSE3* B, PslSE3* C) {
    double r[3];
    psl_po_rotate(A->q, B->t, r);
    const double *a = A->q, *b = B->q;
    double q[4];
    q[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    q[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    q[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    q[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    psl_po_normalize(q);
    for (int i = 0; i < 4; ++i) C->q[i] = q[i];
    for (int i = 0; i < 3; ++i) C->t[i] = A->t[i] + r[i];
}

// computeError of both edges at pose T: e (e[2] = 0 for a monocular edge), the camera point Pc; returns 1 for a monocular edge.
// E: u v ur inv_sigma2 x y z.  The stereo projection keeps its `const float invz` (types_six_dof_expmap.cpp:300).
PSL_PO_HD int psl_po_error(const float* E, const PslSE3* T, const PslPoseCamD* K, double* e, double* Pc) {
    const double Xw[3] = {(double)E[4], (double)E[5], (double)E[6]};
    double r[3];
    psl_po_rotate(T->q, Xw, r);
    Pc[0] = r[0] + T->t[0]; Pc[1] = r[1] + T->t[1]; Pc[2] = r[2] + T->t[2];
    const int mono = E[2] < 0.f;
    if (mono) {
        e[0] = (double)E[0] - (PSL_PO_DIV(Pc[0], Pc[2]) * K->fx + K->cx);
        e[1] = (double)E[1] - (PSL_PO_DIV(Pc[1], Pc[2]) * K->fy + K->cy);
        e[2] = 0.0;
    } else {
        const double invz = (double)(float)PSL_PO_DIV(1.0, Pc[2]);
        const double r0 = (Pc[0] * invz) * K->fx + K->cx;
        e[0] = (double)E[0] - r0;
        e[1] = (double)E[1] - ((Pc[1] * invz) * K->fy + K->cy);
        e[2] = (double)E[2] - (r0 - K->bf * invz);
    }
    return mono;
}

// chi2 = e . (invSigma2 I) e
PSL_PO_HD double psl_po_chi2(const double* e, double is2, int mono) {
    const double c = e[0] * (is2 * e[0]) + e[1] * (is2 * e[1]);
    return mono ? c : c + e[2] * (is2 * e[2]);
}

// linearizeOplus (types_six_dof_expmap.cpp:266-288, :335-364) and constructQuadraticForm (base_unary_edge.hpp:43-72) of one edge:
// adds its 28 terms to acc.  w = rho' * invSigma2 weighs both H and b.
PSL_PO_HD void psl_po_add_terms(const double* e, const double* Pc, int mono, double is2, double rho0, double rho1, const PslPoseCamD* K,
                                double* acc) {
    const double x = Pc[0], y = Pc[1], invz = PSL_PO_DIV(1.0, Pc[2]), invz2 = invz * invz;
    double J[3][6];
    J[0][0] = ((x * y) * invz2) * K->fx;
    J[0][1] = (-(1.0 + (x * x) * invz2)) * K->fx;
    J[0][2] = (y * invz) * K->fx;
    J[0][3] = (-invz) * K->fx;
    J[0][4] = 0.0;
    J[0][5] = (x * invz2) * K->fx;
    J[1][0] = (1.0 + (y * y) * invz2) * K->fy;
    J[1][1] = (((-x) * y) * invz2) * K->fy;
    J[1][2] = ((-x) * invz) * K->fy;
    J[1][3] = 0.0;
    J[1][4] = (-invz) * K->fy;
    J[1][5] = (y * invz2) * K->fy;
    J[2][0] = J[0][0] - (K->bf * y) * invz2;
    J[2][1] = J[0][1] + (K->bf * x) * invz2;
    J[2][2] = J[0][2];
    J[2][3] = J[0][3];
    J[2][4] = 0.0;
    J[2][5] = J[0][5] - K->bf * invz2;
    const double w = rho1 * is2;
    int h = 0;
    for (int j = 0; j < 6; ++j) {
        const double w0 = w * J[0][j], w1 = w * J[1][j], w2 = w * J[2][j];
        for (int k = j; k < 6; ++k, ++h) {
            const double s = w0 * J[0][k] + w1 * J[1][k];
            acc[h] = acc[h] + (mono ? s : s + w2 * J[2][k]);
        }
        const double s = w0 * e[0] + w1 * e[1];
        acc[21 + j] = acc[21 + j] + (mono ? s : s + w2 * e[2]);
    }
    acc[27] = acc[27] + rho0;
}

// ---- the LIL edge: EdgeLILSE3ProjectXYZ with its fixed VertexLIL (add_inc/EdgeLIL.h:210-439, src/Optimizer.cc:619-694) ---------------
// One row L of 23 doubles (PslPoseLilEdge): the world data X1s X1e X2s X2e Xins (L[0..14]: line1 start / end, line2 start / end,
// crosspoint) and the observation l1 l2 ins (L[15..22]: mvle_l[i].first, .second, CrossPoint_2D[i]).  Information: the identity
// (invSigma = 1, src/Optimizer.cc:241, :668).  The vertex is fixed, so only _jacobianOplusXj (:339-379) enters H and b.
#define PSL_POSE_LIL_DOUBLES 23
#define PSL_POSE_DELTA_LIL 3.3271608352661133   /* float deltaLJL = sqrt(11.07) (src/Optimizer.cc:628) */

// T.map(X) and cam_project of it (EdgeLIL.h:415-430: project2d divides, then * fx + cx)
PSL_PO_HD void psl_po_lil_map(const double* X, const PslSE3* T, double* Pc) {
    double r[3];
    psl_po_rotate(T->q, X, r);
    Pc[0] = r[0] + T->t[0]; Pc[1] = r[1] + T->t[1]; Pc[2] = r[2] + T->t[2];
}
PSL_PO_HD void psl_po_lil_project(const double* X, const PslSE3* T, const PslPoseCamD* K, double* uv) {
    double Pc[3];
    psl_po_lil_map(X, T, Pc);
    uv[0] = PSL_PO_DIV(Pc[0], Pc[2]) * K->fx + K->cx;
    uv[1] = PSL_PO_DIV(Pc[1], Pc[2]) * K->fy + K->cy;
}

// computeError (EdgeLIL.h:220-256): e0, e1 = (u, v, 1) . l1 at X1s, X1e; e2, e3 = (u, v, 1) . l2 at X2s, X2e; (e4, e5) = ins - P(Xins).
// The products of the 2x3 matrix with the line run in index order; 1.0 * l[2] is l[2].
PSL_PO_HD void psl_po_lil_error(const double* L, const PslSE3* T, const PslPoseCamD* K, double* e) {
    double uv[2];
    for (int r = 0; r < 4; ++r) {
        const double* l = L + 15 + 3 * (r >> 1);
        psl_po_lil_project(L + 3 * r, T, K, uv);
        e[r] = (uv[0] * l[0] + uv[1] * l[1]) + l[2];
    }
    psl_po_lil_project(L + 12, T, K, uv);
    e[4] = L[21] - uv[0];
    e[5] = L[22] - uv[1];
}

// chi2 = e . (1.0 I) e, the six products summed in ascending order
PSL_PO_HD double psl_po_lil_chi2(const double* e) {
    double c = e[0] * e[0];
    for (int r = 1; r < 6; ++r) c = c + e[r] * e[r];
    return c;
}

// a line row of _jacobianOplusXj (EdgeLIL.h:339-365) at the camera point Pc with the line (l0, l1), every entry in the header's order
PSL_PO_HD void psl_po_lil_row_line(const double* Pc, double l0, double l1, const PslPoseCamD* K, double* J) {
    const double x = Pc[0], y = Pc[1], invz = PSL_PO_DIV(1.0, Pc[2]), invz2 = invz * invz;
    const double fx = K->fx, fy = K->fy;
    J[0] = ((((-fx) * x) * y) * invz2) * l0 - (fy * (1.0 + (y * y) * invz2)) * l1;
    J[1] = (fx * (1.0 + (x * x) * invz2)) * l0 + (((fy * x) * y) * invz2) * l1;
    J[2] = (((-fx) * y) * invz) * l0 + ((fy * x) * invz) * l1;
    J[3] = (fx * invz) * l0;
    J[4] = (fy * invz) * l1;
    J[5] = (((-fx) * x) * l0 - (fy * y) * l1) * invz2;
}

// rows 4 and 5 (EdgeLIL.h:367-379): the monocular point edge's rows at Xins, in this header's order
PSL_PO_HD void psl_po_lil_row_ins(const double* Pc, int second, const PslPoseCamD* K, double* J) {
    const double x = Pc[0], y = Pc[1], invz = PSL_PO_DIV(1.0, Pc[2]), invz2 = invz * invz;
    const double fx = K->fx, fy = K->fy;
    if (!second) {
        J[0] = ((x * y) * invz2) * fx;
        J[1] = (-(1.0 + (x * x) * invz2)) * fx;
        J[2] = (y * invz) * fx;
        J[3] = (-fx) * invz;
        J[4] = 0.0;
        J[5] = (x * invz2) * fx;
    } else {
        J[0] = (1.0 + (y * y) * invz2) * fy;
        J[1] = (((-fy) * x) * y) * invz2;
        J[2] = ((-fy) * x) * invz;
        J[3] = 0.0;
        J[4] = (-fy) * invz;
        J[5] = (fy * y) * invz2;
    }
}

// the rank-one contribution of one Jacobian row J with its error er: acc_H[jk] += (w J_j) J_k, acc_b[j] += (w J_j) er
PSL_PO_HD void psl_po_lil_add_row(const double* J, double er, double w, double* acc) {
    int h = 0;
    for (int j = 0; j < 6; ++j) {
        const double wj = w * J[j];
        for (int k = j; k < 6; ++k, ++h) acc[h] = acc[h] + wj * J[k];
        acc[21 + j] = acc[21 + j] + wj * er;
    }
}

// linearizeOplus (EdgeLIL.h:264-381) and constructQuadraticForm of one LIL edge: adds its 28 terms to acc row by row - row 0, its
// rank-one contribution, row 1, ... row 5, then rho - so that no 6x6 Jacobian is ever live.  w = rho' (the information is 1.0).
// linearizeOplus reads segment<3>(9) for xyz2_s AND xyz2_e (:273-275): row 2 of the Jacobian is evaluated at the END point of line 2
// while e[2] is the error at its START point.  That is the reference's behaviour and is kept.
PSL_PO_HD void psl_po_lil_add_terms(const double* L, const double* e, const PslSE3* T, double rho0, double rho1, const PslPoseCamD* K,
                                    double* acc) {
    double Pc[3], J[6];
    for (int r = 0; r < 4; ++r) {
        const double* l = L + 15 + 3 * (r >> 1);
        psl_po_lil_map(L + (r == 2 ? 9 : 3 * r), T, Pc);
        psl_po_lil_row_line(Pc, l[0], l[1], K, J);
        psl_po_lil_add_row(J, e[r], rho1, acc);
    }
    psl_po_lil_map(L + 12, T, Pc);
    for (int r = 4; r < 6; ++r) {
        psl_po_lil_row_ins(Pc, r - 4, K, J);
        psl_po_lil_add_row(J, e[r], rho1, acc);
    }
    acc[27] = acc[27] + rho0;
}

// The estimate of a pose `Problem` and its candidate: the vertex part of what psl_lm_optimize<6> asks for.
struct PslPoseVertex {
    PslSE3 T, Tn;
    const double* sctab;   // the table of psl_sincos_glibc.h
    PSL_LM_MEMBER void candidate(double* x) {
        PslSE3 dT;
        psl_po_exp(x, &dT, sctab);
        psl_po_mul(&dT, &T, &Tn);   // oplusImpl: exp(update) * estimate
    }
    PSL_LM_MEMBER void accept() { T = Tn; }
};

// The four rounds of PoseOptimization on one vertex, each one optimize(10) (psl_lm_optimize<6>).  Problem is a PslPoseVertex that
// also supplies what is summed over the edges (in its own, fixed order) and takes the results of a round:
//   int round, bool robust             set here: the round index - from round 1 on an edge whose outlier byte is set is not active -
//                                      and whether the Huber kernel is on
//   sums(acc)                          the 28 sums (PSL_POSE_NTERMS) of the active edges at T
//   chi()                              the robust chi2 of the active edges at Tn
//   classify(&nbad, &nbad_lil)         the outlier bytes of ALL edges at T and the count of either kind
//   round_done(r, its)                 round r has run its iterations (PslPoseInfo)
// nt: the edges of both kinds, at least 3.  T_out: the pose of the last round; nbad_out: its outlying POINT edges -
// nInitialCorrespondences - nBad (:1022) counts an outlying LIL edge as good.
template <class Problem>
PSL_PO_HD void psl_po_rounds(Problem& P, const PslSE3& T0, int nt, PslSE3* T_out, int* nbad_out) {
    int nbad = 0, nbad_lil = 0;
    for (int r = 0; r < 4; ++r) {
        P.round = r;
        P.T = T0;                 // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) (:719)
        P.robust = r < 3;         // e->setRobustKernel(0) after round index 2 (:749)
        // without an active edge g2o has no vertex to optimise and optimize() returns at once
        const int its = nt - nbad - nbad_lil > 0 ? psl_lm_optimize<6>(P, 10) : 0;
        // the plain chi2 of every edge at the round's pose, as a float, against 5.991f / 7.815f (:724-780) and of every LIL edge
        // against 11.07f (:977-1008)
        P.classify(&nbad, &nbad_lil);
        P.round_done(r, its);
        if (nt < 10) break;   // optimizer.edges().size() < 10: all edges, not the active ones (:1011)
    }
    *T_out = P.T;
    *nbad_out = nbad;
}

#endif
