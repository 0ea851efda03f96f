// Optimizer::OptimizeSim3 (pslfe_sim3.hip) as functions of one thread: Sim3 and its exponential, the two projection errors of a
// pair, g2o's numeric Jacobian, the quadratic form, the Sim3 update and psl_s3_rounds (the two optimize() calls - each one
// psl_lm_optimize<7> of lm_kernels.h, which holds the Levenberg loop and the 7x7 solve -, the removal of outlying pairs between
// them, the early return, the final count).  Product code.  Plain C++ text: the kernel includes it for the device and
// tools/dropin/sim3_main.cpp for its host loop, so both run the same single IEEE operations (build with -ffp-contract=off).
// psl_s3_rounds asks its `Problem` argument for everything that is summed over the pairs; the order of those sums is not here but
// in the `Problem`.  The host loop instantiates psl_s3_rounds; k_sim3_optimize holds it and the driver's loop written out (the header
// of pslfe_sim3.hip says why), so they are changed together.  Restated from the reference:
//   Sim3: constructors, exp, map, inverse, product   Thirdparty/g2o/g2o/types/sim3.h:59-67, :70-142, :144, :233-236, :266-272
//   oplusImpl, the two errors                        Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:60-69, :138-145, :160-167
//   project                                          Thirdparty/g2o/g2o/types/se3_ops.hpp:49-55
//   the numeric Jacobian, the quadratic form         Thirdparty/g2o/g2o/core/base_binary_edge.hpp:131-205, :55-120
//   the calls, the classification, the return        src/Optimizer.cc:2801-2996
// linearizeOplus of both edges is commented out in the reference (types_seven_dof_expmap.h:147, :169), so g2o differentiates by
// central differences with delta = 1e-9; that is the reference's behaviour and is restated as it is.  A one-ulp difference in an
// error becomes a 1e-5 relative difference in a Jacobian entry: the kernel, the host loop and the numpy restatement
// (tests/sim3_opt_cases.py) must agree in every operation.
// Eigen is not in the reference tree, so where g2o hands a step to Eigen the order written here is this library's: sums run in
// index order, left to right.  Parity with g2o itself is unpinned.
// sin / cos are psl_glibc_sin / psl_glibc_cos; exp is psl_exp (fdlibm's, at most one ulp off glibc's: psl_f64math.h).
#ifndef PSL_SIM3_KERNELS_H
#define PSL_SIM3_KERNELS_H

#include "pose_kernels.h"

#ifndef PSL_F64_QUAL
#define PSL_F64_QUAL PSL_PO_HD
#endif
#include "psl_f64math.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

// full unrolling keeps the small arrays below in registers on the device (indices become constants)
#define PSL_S3_UNROLL PSL_LM_UNROLL

// On the device the perturbed estimates of column d are read through an offset of 0 that the compiler cannot see through and that
// depends on column d - 1 (no instruction is emitted): without it the scheduler loads all 14 estimates of an edge at once, 224 live
// registers next to the 36 accumulators, and spills (profiles/sim3_codegen.txt).  It changes no arithmetic.
#if defined(__HIP_DEVICE_COMPILE__)
#define PSL_S3_AFTER(z, val) asm volatile("" : "+v"(z) : "v"(val))
#else
#define PSL_S3_AFTER(z, val) (void)(val)
#endif

#define PSL_S3_NTERMS 36     // per pair: the 28 upper-triangle values of H row by row, the 7 of b (before the sign), the robust chi2
#define PSL_S3_NPERT 14      // the perturbed estimates of one linearisation: +delta e_d (index 2d) and -delta e_d (2d + 1), d = 0..6
#define PSL_S3_PAIR_FLOATS 12
#define PSL_S3_DELTA 1e-9                    // base_binary_edge.hpp:147
#define PSL_S3_SCALAR (1.0 / (2 * 1e-9))     // :148

struct PslS3 {
    double q[4];   // x y z w, NOT normalised: neither Quaterniond(R) nor a product normalises (sim3.h:64-67, :268)
    double t[3];
    double s;
};

struct PslS3Cams {
    double fx1, fy1, cx1, cy1, fx2, fy2, cx2, cy2;
};

// Sim3(R, t, s) (sim3.h:64-67) from the floats Sim3Solver hands over (src/LoopClosing.cc:320-325)
PSL_PO_HD void psl_s3_from_rts(const float* R9, const float* t3, float s, PslS3* S) {
    double R[9];
    for (int i = 0; i < 9; ++i) R[i] = (double)R9[i];
    psl_po_quat_from_R(R, S->q);
    for (int i = 0; i < 3; ++i) S->t[i] = (double)t3[i];
    S->s = (double)s;
}

// Sim3(update) (sim3.h:70-142): update = (omega, upsilon, sigma); the four branches on |sigma| < 1e-5 and theta < 1e-5.
// *branch (may be NULL) = (|sigma| >= eps) * 2 + (theta >= eps).
PSL_PO_HD void psl_s3_exp(const double* x, PslS3* S, const double* tab, int* branch) {
    const double sigma = x[6];
    const double theta = PSL_PO_SQRT((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    const double O[9] = {0.0, -x[2], x[1], x[2], 0.0, -x[0], -x[1], x[0], 0.0};
    const double s = psl_exp(sigma);
    double O2[9], R[9];
    psl_po_mat3mul(O, O, O2);
    const double eps = 0.00001;
    double A, B, C;
    const int big_sigma = !(__builtin_fabs(sigma) < eps), big_theta = !(theta < eps);
    if (big_theta) {   // R = I + sin(theta)/theta Omega + (1 - cos(theta))/(theta*theta) Omega2 (:106, :121)
        const double sn = psl_glibc_sin(theta, tab), cs = psl_glibc_cos(theta, tab);
        const double a = PSL_PO_DIV(sn, theta), b = PSL_PO_DIV(1.0 - cs, theta * theta);
        for (int i = 0; i < 9; ++i) R[i] = (((i % 4) == 0 ? 1.0 : 0.0) + a * O[i]) + b * O2[i];
        if (!big_sigma) {
            const double theta2 = theta * theta;
            C = 1.0;
            A = PSL_PO_DIV(1.0 - cs, theta2);
            B = PSL_PO_DIV(theta - sn, theta2 * theta);
        } else {
            C = PSL_PO_DIV(s - 1.0, sigma);
            const double sa = s * sn, sb = s * cs;
            const double theta2 = theta * theta, sigma2 = sigma * sigma;
            const double c = theta2 + sigma2;
            A = PSL_PO_DIV(sa * sigma + (1.0 - sb) * theta, theta * c);
            B = PSL_PO_DIV(C - PSL_PO_DIV((sb - 1.0) * sigma + sa * theta, c), theta2);   // (C - ...) * 1. / theta2: * 1. changes no bit
        }
    } else {           // R = I + Omega + Omega*Omega (:99, :117)
        for (int i = 0; i < 9; ++i) R[i] = (((i % 4) == 0 ? 1.0 : 0.0) + O[i]) + O2[i];
        if (!big_sigma) {
            C = 1.0;
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            C = PSL_PO_DIV(s - 1.0, sigma);
            const double sigma2 = sigma * sigma;
            A = PSL_PO_DIV((sigma - 1.0) * s + 1.0, sigma2);
            B = PSL_PO_DIV(((0.5 * sigma2 - sigma) + 1.0) * s, sigma2 * sigma);
        }
    }
    if (branch) *branch = big_sigma * 2 + big_theta;
    psl_po_quat_from_R(R, S->q);
    // W = A Omega + B Omega2 + C I; t = W upsilon (:140-141)
    double W[9];
    for (int i = 0; i < 9; ++i) W[i] = (A * O[i] + B * O2[i]) + C * ((i % 4) == 0 ? 1.0 : 0.0);
    for (int i = 0; i < 3; ++i) S->t[i] = (W[3 * i] * x[3] + W[3 * i + 1] * x[4]) + W[3 * i + 2] * x[5];
    S->s = s;
}

// Sim3::map (:144): s (r xyz) + t
PSL_PO_HD void psl_s3_map(const PslS3* S, const double* X, double* o) {
    double r[3];
    psl_po_rotate(S->q, X, r);
    o[0] = S->s * r[0] + S->t[0]; o[1] = S->s * r[1] + S->t[1]; o[2] = S->s * r[2] + S->t[2];
}

// Sim3::inverse (:233-236): Sim3(r.conjugate(), r.conjugate() * ((-1. / s) * t), 1. / s)
PSL_PO_HD void psl_s3_inverse(const PslS3* S, PslS3* I) {
    const double qc[4] = {-S->q[0], -S->q[1], -S->q[2], S->q[3]};
    const double m = PSL_PO_DIV(-1.0, S->s);
    const double v[3] = {m * S->t[0], m * S->t[1], m * S->t[2]};
    double r[3];
    psl_po_rotate(qc, v, r);
    for (int i = 0; i < 4; ++i) I->q[i] = qc[i];
    for (int i = 0; i < 3; ++i) I->t[i] = r[i];
    I->s = PSL_PO_DIV(1.0, S->s);
}

// Sim3::operator* (:266-272): A * B, the quaternion product in Eigen's order and not normalised
PSL_PO_HD void psl_s3_mul(const PslS3* A, const PslS3* B, PslS3* C) {
    double r[3];
    psl_po_rotate(A->q, B->t, r);
    const double *a = A->q, *b = B->q;
    double q[4];
    q[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    q[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    q[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    q[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
    const double s = A->s * B->s;
    for (int i = 0; i < 3; ++i) C->t[i] = A->s * r[i] + A->t[i];
    for (int i = 0; i < 4; ++i) C->q[i] = q[i];
    C->s = s;
}

// VertexSim3Expmap::oplusImpl (types_seven_dof_expmap.h:60-69): update[6] = 0 with a fixed scale, then Sim3(update) * estimate.
// With a fixed scale exp(0) = 1 and 1 * s = s: the scale keeps its bits.
PSL_PO_HD void psl_s3_oplus(const double* x, int fix_scale, const PslS3* S, const double* tab, PslS3* Sn, int* branch) {
    double u[7];
    for (int i = 0; i < 7; ++i) u[i] = x[i];
    if (fix_scale) u[6] = 0.0;
    PslS3 d;
    psl_s3_exp(u, &d, tab, branch);
    psl_s3_mul(&d, S, Sn);
}

// Perturbed estimate k of the linearisation at S (base_binary_edge.hpp:176-198): oplus(+delta e_d) for k = 2d, oplus(-delta e_d) for
// k = 2d + 1, and its inverse, which EdgeInverseSim3ProjectXYZ::computeError forms.  A function of the estimate alone.
PSL_PO_HD void psl_s3_perturbed(const PslS3* S, int k, int fix_scale, const double* tab, PslS3* Sp, PslS3* Spi) {
    double u[7];
    PSL_S3_UNROLL
    for (int d = 0; d < 7; ++d) u[d] = d != (k >> 1) ? 0.0 : (k & 1) ? -PSL_S3_DELTA : PSL_S3_DELTA;
    psl_s3_oplus(u, fix_scale, S, tab, Sp, nullptr);
    psl_s3_inverse(Sp, Spi);
}

// obs - cam_map(project(S.map(X))) (types_seven_dof_expmap.h:144, :166; se3_ops.hpp:49-55: the two divisions by z)
PSL_PO_HD void psl_s3_error(const PslS3* S, const double* X, double u, double v, double fx, double fy, double cx, double cy, double* e) {
    double P[3];
    psl_s3_map(S, X, P);
    e[0] = u - (PSL_PO_DIV(P[0], P[2]) * fx + cx);
    e[1] = v - (PSL_PO_DIV(P[1], P[2]) * fy + cy);
}

// A pair row P (PslSim3Pair, 12 floats): u1 v1 inv_sigma2_1 u2 v2 inv_sigma2_2 P1c[3] P2c[3].
// side 0: the e12 edge, obs1 - cam_map1(project(S12.map(P2c))); side 1: the e21 edge, obs2 - cam_map2(project(S12^-1.map(P1c))).
// S is S12 for side 0 and its inverse for side 1.
PSL_PO_HD void psl_s3_edge_error(const float* P, int side, const PslS3* S, const PslS3Cams* K, double* e) {
    if (!side) {
        const double X[3] = {(double)P[9], (double)P[10], (double)P[11]};
        psl_s3_error(S, X, (double)P[0], (double)P[1], K->fx1, K->fy1, K->cx1, K->cy1, e);
    } else {
        const double X[3] = {(double)P[6], (double)P[7], (double)P[8]};
        psl_s3_error(S, X, (double)P[3], (double)P[4], K->fx2, K->fy2, K->cx2, K->cy2, e);
    }
}

// chi2 = e . (invSigma2 I) e
PSL_PO_HD double psl_s3_chi2(const double* e, double is2) { return e[0] * (is2 * e[0]) + e[1] * (is2 * e[1]); }

// The delta of psl_lm_huber is `const float deltaHuber = sqrt(th2)` (src/Optimizer.cc:2850).  th2 is a float and <cmath> is in scope
// there, so this is the FLOAT root, std::sqrt(float), widened to double by setDelta: PSL_S3_HUBER_DELTA.  (For th2 = 10, what
// LoopClosing passes, the float root and the rounded double root are the same float.)
#define PSL_S3_HUBER_DELTA(th2) ((double)__builtin_sqrtf(th2))

// One edge of a pair at the estimate S (Si = its inverse): the error e (out), the weight w = rho' * invSigma2 that weighs both H
// and b (out), and the edge's robust chi2 (returned).
PSL_PO_HD double psl_s3_edge_rho(const float* P, int side, const PslS3* S, const PslS3* Si, const PslS3Cams* K, double delta, double* e,
                                 double* w) {
    psl_s3_edge_error(P, side, side ? Si : S, K, e);
    const double is2 = (double)P[side ? 5 : 2];
    const double c = psl_s3_chi2(e, is2);
    double rho0, rho1;
    psl_lm_huber(c, delta, &rho0, &rho1);
    *w = rho1 * is2;
    return rho0;
}

// linearizeOplus and constructQuadraticForm of one edge: the numeric Jacobian from the perturbed estimates pert[k][0] (Sp) /
// pert[k][1] (Spi) - column d is scalar * (e(+delta e_d) - e(-delta e_d)) - and the edge's 36 terms added to acc.
PSL_PO_HD void psl_s3_edge_terms(const float* P, int side, const PslS3* S, const PslS3* Si, const PslS3 (*pert)[2], const PslS3Cams* K,
                                 double delta, double* acc) {
    double e[2], w;
    const double rho0 = psl_s3_edge_rho(P, side, S, Si, K, delta, e, &w);
    double J[2][7];
    int z = 0;
    PSL_S3_AFTER(z, rho0);
    PSL_S3_UNROLL
    for (int d = 0; d < 7; ++d) {
        double ep[2], em[2];
        psl_s3_edge_error(P, side, &pert[2 * d + z][side], K, ep);
        psl_s3_edge_error(P, side, &pert[2 * d + 1 + z][side], K, em);
        J[0][d] = PSL_S3_SCALAR * (ep[0] - em[0]);
        J[1][d] = PSL_S3_SCALAR * (ep[1] - em[1]);
        PSL_S3_AFTER(z, J[1][d]);
    }
    int h = 0;
    PSL_S3_UNROLL
    for (int j = 0; j < 7; ++j) {
        const double w0 = w * J[0][j], w1 = w * J[1][j];
        PSL_S3_UNROLL
        for (int k = j; k < 7; ++k, ++h) acc[h] = acc[h] + (w0 * J[0][k] + w1 * J[1][k]);
        acc[28 + j] = acc[28 + j] + (w0 * e[0] + w1 * e[1]);
    }
    acc[35] = acc[35] + rho0;
}

// the plain chi2 of both edges of a pair against (double)th2 (src/Optimizer.cc:2948, :2982): no cast to float
PSL_PO_HD int psl_s3_pair_bad(const float* P, const PslS3* S, const PslS3* Si, const PslS3Cams* K, double th2) {
    double e[2];
    psl_s3_edge_error(P, 0, S, K, e);
    const double c12 = psl_s3_chi2(e, (double)P[2]);
    psl_s3_edge_error(P, 1, Si, K, e);
    const double c21 = psl_s3_chi2(e, (double)P[5]);
    return (c12 > th2 || c21 > th2) ? 1 : 0;
}

// The estimate of a Sim3 `Problem` and its candidate, each used with its inverse: the vertex part of what psl_lm_optimize<7> asks for.
struct PslS3Vertex {
    PslS3 T, Tn;
    int fix_scale;
    int branches;          // bit k set when a trial step took branch k of the exponential
    const double* sctab;   // the table of psl_sincos_glibc.h
    // With a fixed scale oplusImpl writes 0 into the solver's own x[6] (types_seven_dof_expmap.h:62-65, the const_cast), so
    // computeScale sees it: x[6] is cleared here too.
    PSL_LM_MEMBER void candidate(double* x) {
        if (fix_scale) x[6] = 0.0;
        int br = 0;
        psl_s3_oplus(x, fix_scale, &T, sctab, &Tn, &br);
        branches |= 1 << br;
    }
    PSL_LM_MEMBER void accept() { T = Tn; }
};

// The two optimize() calls of OptimizeSim3 on one vertex.  Problem is a PslS3Vertex that also supplies what is summed over the pairs
// (in its own, fixed order):
//   sums(acc)                    the 36 sums (PSL_S3_NTERMS) of the active pairs at T; the Problem forms the 14 perturbed estimates
//                                of the linearisation (psl_s3_perturbed) once, not per edge
//   chi()                        the robust chi2 of the active pairs at Tn
//   classify()                   tests every ACTIVE pair at T, sets the outlier byte of an outlying one (which makes it inactive)
//                                and returns how many it set
//   call_done(c, its)            call c has run its iterations (PslSim3Info)
// The Huber kernel is on in both calls; the estimate carries over from the first call to the second; lambda, ni and _nBad are
// re-initialised by each call.  Returns the return value of OptimizeSim3; *written = 0 when the reference returns before writing
// g2oS12 back (:2966), and S_out is then S0.
template <class Problem>
PSL_PO_HD int psl_s3_rounds(Problem& P, const PslS3& S0, int npairs, PslS3* S_out, int* written) {
    *S_out = S0;
    *written = 0;
    P.branches = 0;
    if (npairs <= 0) return 0;   // no edge: nothing to optimise, nCorrespondences - nBad < 10
    P.T = S0;
    const int its0 = psl_lm_optimize<7>(P, 5);           // optimizer.optimize(5) (:2937)
    P.call_done(0, its0);
    const int nbad = P.classify();                       // :2940-2958: the outlying pairs leave
    const int more = nbad > 0 ? 10 : 5;                  // :2960-2964
    if (npairs - nbad < 10) return 0;                    // :2966: g2oS12 is not written
    const int its1 = psl_lm_optimize<7>(P, more);        // :2972, from the estimate the first call left
    P.call_done(1, its1);
    const int nbad2 = P.classify();                      // :2974-2989
    *S_out = P.T;
    *written = 1;
    return npairs - nbad - nbad2;                        // nIn
}

#endif
