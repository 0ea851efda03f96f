// Optimizer::OptimizeEssentialGraph (pslfe_essential.hip): the measurements of the edges, Sim3::log, EdgeSim3 with g2o's numeric
// Jacobian, the 7x7 blocks of the quadratic form, an LDLt on the lower triangle stored by row envelopes, g2o's Levenberg loop from
// the user's lambda, the pose recovery and the map point correction.  Product code.  Plain C++ text: k_eg_optimize includes it for
// the device and tools/dropin/essential_main.cpp for one core, so both run the same single IEEE operations (build with
// -ffp-contract=off; division and square root are PSL_LM_DIV / PSL_LM_SQRT, sin / cos the restated tables of psl_sincos_glibc.h,
// log / exp / acos those of psl_f64math.h, no device math library).  tests/essential_cases.py is the same text in Python.
//
// One text for both, as ba_kernels.h: every step is a function of (workspace, index) that writes only what the index owns, and
// psl_eg_run is a template over an executor `Exec` (par / one / sum256 / get: the contract is in lm_kernels.h above
// psl_lm_levenberg, the Levenberg driver, which PslEgProblem gives its steps).  PslLmSerial runs the steps on one core,
// PslLmWorkgroup of lm_device.h on the 256 threads of a workgroup with a barrier after each.  No step depends on how its indices
// are spread, so the two equal each other bit for bit by construction.
//
// Restated from the reference:
//   the vertices, the measurements, the call          src/Optimizer.cc:2564-2599, :2607-2738, :2741-2742
//   the poses and the points afterwards               src/Optimizer.cc:2747-2798
//   Sim3::log                                         Thirdparty/g2o/g2o/types/sim3.h:148-230; deltaR, skew se3_ops.hpp:27-47
//   EdgeSim3::computeError                            Thirdparty/g2o/g2o/types/types_seven_dof_expmap.h:106-114
//   the numeric Jacobian, the quadratic form          Thirdparty/g2o/g2o/core/base_binary_edge.hpp:131-205, :55-120
//   Levenberg with setUserLambdaInit(1e-16)           core/optimization_algorithm_levenberg.cpp:61-189
// Pinned to the reference's text: which Sim3 enters a measurement, C * v1 * v2^-1 from left to right, the four branches of log and
// their formulas, delta = 1e-9 and the central differences of every free vertex half (a fixed half is skipped), information I7,
// no robust kernel, update[6] = 0 with a fixed scale inside oplusImpl only (the column stays in the system and computeScale sees
// the cleared entry), lambda from 1e-16, 20 iterations in one optimize() call, t * (1. / s), the float casts of toCvSE3 / toCvMat,
// Srw = the vertex's FIRST estimate and correctedSwr = the inverse of its last one.
// This library's reading (Eigen is not in the reference tree): sums run in index order, left to right; B*Omega*Omega is
// (B Omega) Omega; W.lu().solve(t) is psl_eg_lu3 (partial pivoting, the first largest |entry| of the column, elimination of the
// right-hand side along with the rows); chi2 of an edge is sum e_r e_r; a block of H takes its edges in ascending edge index and
// an edge's entry is the sum over its seven rows in ascending row; LinearSolverEigen (a sparse Cholesky behind a fill-reducing
// ordering) is the LDLt without pivoting of psl_ba_solve in the caller's row order, restricted to the row envelopes (below); a
// pivot that is not a finite positive number is "the solve failed", a step that psl_lm_step_ok refuses likewise.
// d < -1 by rounding: acos gives NaN as in the reference; every entry of the error but sigma is then NaN, the chi2 of the trial is
// NaN, rho is NaN: the trial is rejected (`rho > 0` is false), lambda grows, and the trial loop ends (`rho < 0` is false too);
// the iteration counts as run (one without gain for the _nBad rule) and the loop goes on.  sin / cos are not called with a NaN
// angle (their table index is not clamped).
//
// The envelope.  Unknowns: 7 per free keyframe in row order; block row i of the lower triangle is stored from block column
// fb[i] = the lowest free index among i and the free keyframes it shares an edge with, up to the diagonal; every scalar row of the
// block row starts at column 7 fb[i].  The factorisation is the column-at-a-time LDLt of ba_kernels.h: row i >= j of column j
// forms d = A[j][j] - sum_k L[j][k] (L[j][k] D[k]) and s = A[i][j] - sum_k L[i][k] (L[j][k] D[k]) in ascending k, L[i][j] = s / d;
// k runs over the columns inside BOTH envelopes and a row whose envelope starts after j has no entry in column j.  For finite
// input this equals the dense factorisation: an entry outside the envelope of a row is zero in A and, by induction over the
// columns, in L (its s is a sum of products that each have a zero factor), so the terms left out are +-0 and the entries left out
// are +-0.  A signed zero can differ where a running sum is -0 and a term left out would have been -0 (-0 - (-0) = +0): only the
// sign of a zero, which no later sum or comparison sees as a different number.
#ifndef PSL_ESSENTIAL_KERNELS_H
#define PSL_ESSENTIAL_KERNELS_H

#include <stddef.h>

#include "../../include/pslfe.h"
#include "sim3_kernels.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define PSL_EG_HD PSL_LM_HD
#define PSL_EG_ITERATIONS 20       // optimizer.optimize(20) (src/Optimizer.cc:2742)
#define PSL_EG_LAMBDA_INIT 1e-16   // solver->setUserLambdaInit(1e-16) (:2549)
#define PSL_EG_EVALS 15            // work items of an edge's linearisation: its error, then (half, column) with both signs

// The workspace of one graph: views into one block of HBM (host: of one allocation), carved by psl_eg_carve.
struct PslEgWs {
    // the problem
    const PslEgKeyFrame* kf;
    const PslEgEdge* ed;
    const PslMapPointGeom* mp;
    const int32_t* mp_ref;
    int nkf, ne, nmp;
    int fix_scale;
    const double* sctab;
    // estimates, candidates and their inverses; the 14 perturbed estimates of a linearisation, each with its inverse
    PslS3 *S, *Sn, *Si, *Sni;   // [nkf]
    PslS3* pert;                // [nkf][14][2]
    PslS3* meas;                // [ne]
    // per edge: _error, its chi2, _jacobianOplusXi and _jacobianOplusXj ([7 rows][7 columns])
    double *err, *rho0, *Ji, *Jj;   // [ne][7], [ne], [ne][49], [ne][49]
    // the system by free index
    double *Hd, *b, *x, *y, *D;     // [F][49], [7 F] each
    double *Henv, *Lenv;            // the envelope of H and of its factor
    double* scal;                   // [8] values every thread reads back; [8..263] the partial sums of the one-core sum256
    int64_t* roff;                  // [7 F] where scalar row r starts in the envelope
    int32_t *pidx, *kfof, *fb, *lastblk;   // [nkf] free index or -1; [F] its inverse; [F] first block column; [F] last block row of a column
    int32_t *voff, *vlist;          // [nkf + 1], [2 ne]: the (edge, side) items 2 e + side of a keyframe in ascending order
    int32_t* bmask;                 // [ne][15] the log branches an edge's work items took
    int32_t* flag;                  // [8]
};

PSL_EG_HD size_t psl_eg_take(size_t* off, size_t bytes) {
    const size_t at = *off;
    *off = at + ((bytes + 7) & ~(size_t)7);
    return at;
}

// The views of a workspace for the caps (ckf keyframes, ced edges, cenv envelope doubles) at base; returns its size in bytes
// (base may be NULL to ask for it).
PSL_EG_HD size_t psl_eg_carve(char* base, int ckf, int ced, size_t cenv, PslEgWs* W) {
    size_t off = 0;
    const size_t D = sizeof(double), I = sizeof(int32_t), S = sizeof(PslS3), k = (size_t)ckf, e = (size_t)ced;
#define PSL_EG_VIEW(member, type, count) W->member = reinterpret_cast<type*>(base + psl_eg_take(&off, (count)))
    PSL_EG_VIEW(S, PslS3, k * S);
    PSL_EG_VIEW(Sn, PslS3, k * S);
    PSL_EG_VIEW(Si, PslS3, k * S);
    PSL_EG_VIEW(Sni, PslS3, k * S);
    PSL_EG_VIEW(pert, PslS3, 28 * k * S);
    PSL_EG_VIEW(meas, PslS3, e * S);
    PSL_EG_VIEW(err, double, 7 * e * D);
    PSL_EG_VIEW(rho0, double, e * D);
    PSL_EG_VIEW(Ji, double, 49 * e * D);
    PSL_EG_VIEW(Jj, double, 49 * e * D);
    PSL_EG_VIEW(Hd, double, 49 * k * D);
    PSL_EG_VIEW(b, double, 7 * k * D);
    PSL_EG_VIEW(x, double, 7 * k * D);
    PSL_EG_VIEW(y, double, 7 * k * D);
    PSL_EG_VIEW(D, double, 7 * k * D);
    PSL_EG_VIEW(Henv, double, cenv * D);
    PSL_EG_VIEW(Lenv, double, cenv * D);
    PSL_EG_VIEW(scal, double, (8 + PSL_LM_LANES) * D);
    PSL_EG_VIEW(roff, int64_t, 7 * k * sizeof(int64_t));
    PSL_EG_VIEW(pidx, int32_t, k * I);
    PSL_EG_VIEW(kfof, int32_t, k * I);
    PSL_EG_VIEW(fb, int32_t, k * I);
    PSL_EG_VIEW(lastblk, int32_t, k * I);
    PSL_EG_VIEW(voff, int32_t, (k + 1) * I);
    PSL_EG_VIEW(vlist, int32_t, 2 * e * I);
    PSL_EG_VIEW(bmask, int32_t, PSL_EG_EVALS * e * I);
    PSL_EG_VIEW(flag, int32_t, 8 * I);
#undef PSL_EG_VIEW
    return off;
}

PSL_EG_HD void psl_eg_load(const double* r, PslS3* S) {
    for (int i = 0; i < 4; ++i) S->q[i] = r[i];
    for (int i = 0; i < 3; ++i) S->t[i] = r[4 + i];
    S->s = r[7];
}
PSL_EG_HD void psl_eg_store(const PslS3* S, double* r) {
    for (int i = 0; i < 4; ++i) r[i] = S->q[i];
    for (int i = 0; i < 3; ++i) r[4 + i] = S->t[i];
    r[7] = S->s;
}

// W x = t by LU with partial pivoting (the stand-in for W.lu().solve(t), sim3.h:217): in column c the pivot is the first row
// r >= c with the largest |M[r][c]|; the right-hand side is eliminated along with the rows; then the back-substitution, each
// sum left to right.  The swaps are selects, so the rows stay in registers on the device.
PSL_EG_HD void psl_eg_lu3(const double* Wm, const double* t, double* x) {
    double a[4] = {Wm[0], Wm[1], Wm[2], t[0]}, b[4] = {Wm[3], Wm[4], Wm[5], t[1]}, c[4] = {Wm[6], Wm[7], Wm[8], t[2]};
    {   // column 0
        const double fa = __builtin_fabs(a[0]), fb = __builtin_fabs(b[0]), fc = __builtin_fabs(c[0]);
        const int p = (fc > fa && fc > fb) ? 2 : (fb > fa ? 1 : 0);
        PSL_S3_UNROLL
        for (int k = 0; k < 4; ++k) {
            const double pa = a[k], pb = b[k], pc = c[k];
            a[k] = p == 2 ? pc : p == 1 ? pb : pa;
            b[k] = p == 1 ? pa : pb;
            c[k] = p == 2 ? pa : pc;
        }
        const double f1 = PSL_LM_DIV(b[0], a[0]), f2 = PSL_LM_DIV(c[0], a[0]);
        PSL_S3_UNROLL
        for (int k = 1; k < 4; ++k) { b[k] = b[k] - f1 * a[k]; c[k] = c[k] - f2 * a[k]; }
    }
    {   // column 1
        const int p = __builtin_fabs(c[1]) > __builtin_fabs(b[1]);
        PSL_S3_UNROLL
        for (int k = 1; k < 4; ++k) {
            const double pb = b[k], pc = c[k];
            b[k] = p ? pc : pb;
            c[k] = p ? pb : pc;
        }
        const double f = PSL_LM_DIV(c[1], b[1]);
        PSL_S3_UNROLL
        for (int k = 2; k < 4; ++k) c[k] = c[k] - f * b[k];
    }
    x[2] = PSL_LM_DIV(c[3], c[2]);
    x[1] = PSL_LM_DIV(b[3] - b[2] * x[2], b[1]);
    x[0] = PSL_LM_DIV((a[3] - a[1] * x[1]) - a[2] * x[2], a[0]);
}

// Sim3::log (sim3.h:148-230): out = (omega, upsilon, sigma).  *branch (may be NULL) = (|sigma| >= 1e-5) * 2 + !(d > 1 - 1e-5).
// A NaN angle (d outside [-1, 1] or a NaN) gives NaN in omega and upsilon, as the reference's acos, sin and cos do.
PSL_EG_HD void psl_s3_log(const PslS3* S, const double* tab, double* out, int* branch) {
    const double s = S->s;
    const double sigma = psl_log(s);
    double R[9];
    psl_po_quat_to_R(S->q, R);
    const double d = 0.5 * (((R[0] + R[4]) + R[8]) - 1.0);
    const double dR[3] = {R[7] - R[5], R[2] - R[6], R[3] - R[1]};   // deltaR
    const double eps = 0.00001;
    const int big_sigma = !(__builtin_fabs(sigma) < eps), big_theta = !(d > 1.0 - eps);
    if (branch) *branch = big_sigma * 2 + big_theta;
    double om[3], A, B, C;
    if (!big_theta) {
        for (int i = 0; i < 3; ++i) om[i] = 0.5 * dR[i];
        if (!big_sigma) {
            C = 1.0;
            A = 1. / 2.;
            B = 1. / 6.;
        } else {
            C = PSL_LM_DIV(s - 1.0, sigma);
            const double sigma2 = sigma * sigma;
            A = PSL_LM_DIV((sigma - 1.0) * s + 1.0, sigma2);
            B = PSL_LM_DIV(((0.5 * sigma2 - sigma) + 1.0) * s, sigma2 * sigma);
        }
    } else {
        const double theta = psl_acos(d);
        if (!(theta == theta)) {
            for (int i = 0; i < 6; ++i) out[i] = theta;
            out[6] = sigma;
            return;
        }
        const double f = PSL_LM_DIV(theta, 2.0 * PSL_LM_SQRT(1.0 - d * d));
        for (int i = 0; i < 3; ++i) om[i] = f * dR[i];
        const double theta2 = theta * theta;
        const double sn = psl_glibc_sin(theta, tab), cs = psl_glibc_cos(theta, tab);
        if (!big_sigma) {
            C = 1.0;
            A = PSL_LM_DIV(1.0 - cs, theta2);
            B = PSL_LM_DIV(theta - sn, theta2 * theta);
        } else {
            C = PSL_LM_DIV(s - 1.0, sigma);
            const double a = s * sn, bb = s * cs;
            const double c = theta2 + sigma * sigma;
            A = PSL_LM_DIV(a * sigma + (1.0 - bb) * theta, theta * c);
            B = PSL_LM_DIV(C - PSL_LM_DIV((bb - 1.0) * sigma + a * theta, c), theta2);   // (...) * 1. / theta2: * 1. changes no bit
        }
    }
    const double O[9] = {0.0, -om[2], om[1], om[2], 0.0, -om[0], -om[1], om[0], 0.0};   // skew
    double BO[9], BOO[9], Wm[9];
    for (int i = 0; i < 9; ++i) BO[i] = B * O[i];
    psl_po_mat3mul(BO, O, BOO);
    for (int i = 0; i < 9; ++i) Wm[i] = (A * O[i] + BOO[i]) + C * ((i % 4) == 0 ? 1.0 : 0.0);
    psl_eg_lu3(Wm, S->t, out + 3);
    for (int i = 0; i < 3; ++i) out[i] = om[i];
    out[6] = sigma;
}

// EdgeSim3::computeError (types_seven_dof_expmap.h:106-114): log((C * v1) * v2^-1); v2i = v2.inverse()
PSL_EG_HD void psl_eg_error(const PslS3* C, const PslS3* v1, const PslS3* v2i, const double* tab, double* e, int* branch) {
    PslS3 a, m;
    psl_s3_mul(C, v1, &a);
    psl_s3_mul(&a, v2i, &m);
    psl_s3_log(&m, tab, e, branch);
}
PSL_EG_HD double psl_eg_chi2(const double* e) {
    double c = e[0] * e[0];
    for (int r = 1; r < 7; ++r) c = c + e[r] * e[r];
    return c;
}

// The measurement of edge e (src/Optimizer.cc:2612-2622, :2646-2669): a loop edge takes vScw of both ends; any other edge the
// NonCorrectedSim3 entry of an end that has one.  Also clears the edge's branch masks.
PSL_EG_HD void psl_eg_measure(const PslEgWs& W, int e) {
    const PslEgEdge ed = W.ed[e];
    PslS3 Siw, Sjw, Swi;
    psl_eg_load(!ed.loop && W.kf[ed.i].has_nc ? W.kf[ed.i].Snc : W.kf[ed.i].Scw, &Siw);
    psl_eg_load(!ed.loop && W.kf[ed.j].has_nc ? W.kf[ed.j].Snc : W.kf[ed.j].Scw, &Sjw);
    psl_s3_inverse(&Siw, &Swi);
    psl_s3_mul(&Sjw, &Swi, &W.meas[e]);
    for (int h = 0; h < PSL_EG_EVALS; ++h) W.bmask[PSL_EG_EVALS * (size_t)e + h] = 0;
}

// Work item t < 15 nkf of a linearisation: the perturbed estimate t % 15 < 14 of keyframe t / 15 with its inverse (a fixed vertex
// has none), or the inverse of its estimate (t % 15 == 14)
PSL_EG_HD void psl_eg_perturb(const PslEgWs& W, int t) {
    const int v = t / 15, k = t % 15;
    if (k == 14) { psl_s3_inverse(&W.S[v], &W.Si[v]); return; }
    if (W.pidx[v] < 0) return;
    PslS3* p = W.pert + 28 * (size_t)v + 2 * k;
    psl_s3_perturbed(&W.S[v], k, W.fix_scale, W.sctab, p, p + 1);
}

// Work item t < 15 ne of a linearisation (computeActiveErrors and linearizeOplus, base_binary_edge.hpp:131-205): h = t % 15 == 0:
// the edge's error and chi2; else half (h - 1) / 7 (0: vertex i, 1: vertex j) and column d = (h - 1) % 7:
// J[r][d] = (1 / 2e-9) (e(+delta e_d)[r] - e(-delta e_d)[r]).  The half of a fixed vertex is skipped.
PSL_EG_HD void psl_eg_linearize(const PslEgWs& W, int t) {
    const int e = t / PSL_EG_EVALS, h = t % PSL_EG_EVALS;
    const PslEgEdge ed = W.ed[e];
    const PslS3 C = W.meas[e];
    int br = 0, mask = 0;
    if (h == 0) {
        double er[7];
        psl_eg_error(&C, &W.S[ed.i], &W.Si[ed.j], W.sctab, er, &br);
        for (int r = 0; r < 7; ++r) W.err[7 * (size_t)e + r] = er[r];
        W.rho0[e] = psl_eg_chi2(er);
        W.bmask[t] |= 1 << br;
        return;
    }
    const int half = (h - 1) / 7, d = (h - 1) % 7, v = half ? ed.j : ed.i;
    if (W.pidx[v] < 0) return;
    const PslS3* p = W.pert + 28 * (size_t)v + 4 * d;   // [2 d][0], [2 d][1], [2 d + 1][0], [2 d + 1][1]
    double ep[7], em[7];
    if (!half) {
        psl_eg_error(&C, p, &W.Si[ed.j], W.sctab, ep, &br); mask |= 1 << br;
        psl_eg_error(&C, p + 2, &W.Si[ed.j], W.sctab, em, &br); mask |= 1 << br;
    } else {
        psl_eg_error(&C, &W.S[ed.i], p + 1, W.sctab, ep, &br); mask |= 1 << br;
        psl_eg_error(&C, &W.S[ed.i], p + 3, W.sctab, em, &br); mask |= 1 << br;
    }
    double* J = (half ? W.Jj : W.Ji) + 49 * (size_t)e;
    for (int r = 0; r < 7; ++r) J[7 * r + d] = PSL_S3_SCALAR * (ep[r] - em[r]);
    W.bmask[t] |= mask;
}

// the error and chi2 of edge e at the candidates
PSL_EG_HD void psl_eg_trial_error(const PslEgWs& W, int e) {
    const PslEgEdge ed = W.ed[e];
    const PslS3 C = W.meas[e];
    double er[7];
    int br = 0;
    psl_eg_error(&C, &W.Sn[ed.i], &W.Sni[ed.j], W.sctab, er, &br);
    W.rho0[e] = psl_eg_chi2(er);
    W.bmask[PSL_EG_EVALS * (size_t)e] |= 1 << br;
}

// the Jacobian half of item a = 2 e + side, and the other end of its edge
PSL_EG_HD const double* psl_eg_item_J(const PslEgWs& W, int a) { return ((a & 1) ? W.Jj : W.Ji) + 49 * (size_t)(a >> 1); }
PSL_EG_HD int psl_eg_item_other(const PslEgWs& W, int a) { return (a & 1) ? W.ed[a >> 1].i : W.ed[a >> 1].j; }

// One value of the diagonal block or of b of free index t / 56 (constructQuadraticForm, base_binary_edge.hpp:55-120): h = t % 56
// < 49: entry (h / 7, h % 7) = sum over the keyframe's items in ascending order of sum_r J[r][a] J[r][c]; else b[h - 49] =
// -(sum over the items of sum_r J[r][a] e[r])
PSL_EG_HD void psl_eg_build_diag(const PslEgWs& W, int t) {
    const int bi = t / 56, h = t % 56, v = W.kfof[bi];
    const int a = h < 49 ? h / 7 : h - 49, c = h % 7;
    double acc = 0.0;
    for (int q = W.voff[v]; q < W.voff[v + 1]; ++q) {
        const int it = W.vlist[q];
        const double* J = psl_eg_item_J(W, it);
        const double* er = W.err + 7 * (size_t)(it >> 1);
        double s = J[a] * (h < 49 ? J[c] : er[0]);
        for (int r = 1; r < 7; ++r) s = s + J[7 * r + a] * (h < 49 ? J[7 * r + c] : er[r]);
        acc = acc + s;
    }
    if (h < 49) W.Hd[49 * (size_t)bi + h] = acc; else W.b[7 * (size_t)bi + a] = -acc;
}

PSL_EG_HD double* psl_eg_at(const PslEgWs& W, double* env, int r, int c) { return env + W.roff[r] + (c - 7 * W.fb[r / 7]); }

// Column t % 7 of every block of scalar row t / 7 of the envelope of H: the diagonal block's lower triangle from Hd; an
// off-diagonal block (bi, bj), bj < bi, is the sum over the items of keyframe kfof[bi] whose other end is kfof[bj], in ascending
// order, of sum_r Jown[r][a] Jother[r][c] (zero without such an edge)
PSL_EG_HD void psl_eg_build_env(const PslEgWs& W, int t) {
    const int r = t / 7, c = t % 7, bi = r / 7, a = r % 7, v = W.kfof[bi];
    if (c <= a) *psl_eg_at(W, W.Henv, r, 7 * bi + c) = W.Hd[49 * (size_t)bi + 7 * a + c];
    for (int bj = W.fb[bi]; bj < bi; ++bj) {
        const int u = W.kfof[bj];
        double acc = 0.0;
        for (int q = W.voff[v]; q < W.voff[v + 1]; ++q) {
            const int it = W.vlist[q];
            if (psl_eg_item_other(W, it) != u) continue;
            const double *J = psl_eg_item_J(W, it), *Jo = psl_eg_item_J(W, it ^ 1);
            double s = J[a] * Jo[c];
            for (int k = 1; k < 7; ++k) s = s + J[7 * k + a] * Jo[7 * k + c];
            acc = acc + s;
        }
        *psl_eg_at(W, W.Henv, r, 7 * bj + c) = acc;
    }
}

// the two substitutions on one thread: L y = b, then x = D^-1 y - L^T x, each sum in ascending k over the entries inside the envelopes
PSL_EG_HD void psl_eg_substitute(const PslEgWs& W, int N) {
    for (int i = 0; i < N; ++i) {
        double s = W.b[i];
        const int k0 = 7 * W.fb[i / 7];
        const double* row = W.Lenv + W.roff[i];
        for (int k = k0; k < i; ++k) s = s - row[k - k0] * W.y[k];
        W.y[i] = s;
    }
    for (int i = N - 1; i >= 0; --i) {
        double s = PSL_LM_DIV(W.y[i], W.D[i]);
        for (int kb = i / 7; kb <= W.lastblk[i / 7]; ++kb) {   // block rows whose envelope reaches column i, rows k > i in ascending k
            const int k0 = 7 * W.fb[kb];
            if (k0 > i) continue;
            for (int k = 7 * kb > i ? 7 * kb : i + 1; k < 7 * kb + 7; ++k) s = s - W.Lenv[W.roff[k] + (i - k0)] * W.x[k];
        }
        W.x[i] = s;
    }
}

// (H + lambda I) x = b: 1 and x, or 0, "the solve failed"
template <class Exec>
PSL_EG_HD int psl_eg_solve(Exec& X, const PslEgWs& W, int F, double lambda) {
    const int N = 7 * F;
    int32_t* ok = W.flag;
    X.one([&] { *ok = 1; });
    X.par(N, [&](int r) {
        const int k0 = 7 * W.fb[r / 7];
        const double* h = W.Henv + W.roff[r];
        double* l = W.Lenv + W.roff[r];
        for (int k = k0; k < r; ++k) l[k - k0] = h[k - k0];
        l[r - k0] = h[r - k0] + lambda;
    });
    for (int j = 0; j < N; ++j) {
        const int j0 = 7 * W.fb[j / 7];
        const double* rj = W.Lenv + W.roff[j];
        X.par(7 * W.lastblk[j / 7] + 7 - j, [&](int t) {
            const int i = j + t, i0 = 7 * W.fb[i / 7];
            if (i0 > j) return;
            double d = rj[j - j0];
            for (int k = j0; k < j; ++k) d = d - rj[k - j0] * (rj[k - j0] * W.D[k]);
            if (i == j) {
                if (!(d > 0.0) || !(d <= PSL_LM_DBL_MAX)) *ok = 0;
                W.D[j] = d;
                return;
            }
            double* ri = W.Lenv + W.roff[i];
            double s = ri[j - i0];
            for (int k = i0 > j0 ? i0 : j0; k < j; ++k) s = s - ri[k - i0] * (rj[k - j0] * W.D[k]);
            ri[j - i0] = PSL_LM_DIV(s, d);
        });
    }
    if (!X.get(ok)) return 0;
    X.one([&] { psl_eg_substitute(W, N); });
    X.par(F, [&](int i) { if (!psl_lm_step_ok(W.x + 7 * (size_t)i)) *ok = 0; });
    if (!X.get(ok)) return 0;
    return 1;
}

// the partial sum p of 256 of the chi2: the edges p, p + 256, ... in ascending order
PSL_EG_HD double psl_eg_chi_partial(const PslEgWs& W, int p) {
    double s = 0.0;
    for (int e = p; e < W.ne; e += PSL_LM_LANES) s = s + W.rho0[e];
    return s;
}

// The `Problem` of psl_lm_levenberg (lm_kernels.h) for one optimize() call over the F free keyframes.  lambda0: the user's lambda
// (g2o's computeLambdaInit returns it when it is positive).
struct PslEgProblem {
    const PslEgWs& W;
    int F;
    double lambda0;
    template <class Exec> PSL_LM_MEMBER double linearize(Exec& X, double* chi_first) {
        X.par(15 * W.nkf, [&](int t) { psl_eg_perturb(W, t); });
        X.par(PSL_EG_EVALS * W.ne, [&](int t) { psl_eg_linearize(W, t); });
        const double chi = X.sum256([&](int p) { return psl_eg_chi_partial(W, p); });
        if (chi_first) *chi_first = chi;
        X.par(56 * F, [&](int t) { psl_eg_build_diag(W, t); });
        X.par(49 * F, [&](int t) { psl_eg_build_env(W, t); });
        return chi;
    }
    template <class Exec> PSL_LM_MEMBER double lambda_init(Exec&) { return lambda0; }
    template <class Exec> PSL_LM_MEMBER int solve(Exec& X, double lambda) { return psl_eg_solve(X, W, F, lambda); }
    template <class Exec> PSL_LM_MEMBER double candidate(Exec& X) {
        X.par(W.nkf, [&](int v) {       // oplusImpl of every free vertex; with a fixed scale it clears the solver's x[6]
            const int i = W.pidx[v];
            if (i < 0) return;
            double* x = W.x + 7 * (size_t)i;
            if (W.fix_scale) x[6] = 0.0;
            psl_s3_oplus(x, W.fix_scale, &W.S[v], W.sctab, &W.Sn[v], nullptr);
            psl_s3_inverse(&W.Sn[v], &W.Sni[v]);
        });
        X.par(W.ne, [&](int e) { psl_eg_trial_error(W, e); });
        return X.sum256([&](int p) { return psl_eg_chi_partial(W, p); });
    }
    template <class Exec> PSL_LM_MEMBER double scale(Exec& X, double lambda) {
        X.one([&] {                     // computeScale: sum x_j (lambda x_j + b_j) in index order
            double sc = 0.0;
            for (int j = 0; j < 7 * F; ++j) sc = sc + W.x[j] * (lambda * W.x[j] + W.b[j]);
            W.scal[1] = sc;
        });
        return X.get(W.scal + 1);
    }
    template <class Exec> PSL_LM_MEMBER void accept(Exec& X) {
        X.par(W.nkf, [&](int v) {       // discardTop: the candidate becomes the estimate
            if (W.pidx[v] >= 0) { W.S[v] = W.Sn[v]; W.Si[v] = W.Sni[v]; }
        });
    }
};

// Everything of one graph.  `code`: what the caller found in the offsets and the counts (PSLFE_OK, PSLFE_E_CAPACITY, or
// PSLFE_E_INVALID with have == 0 when the offsets name no rows at all); the rows and the envelope are checked here.  A refused
// graph leaves S_out = vScw and mp_out = mp and writes no pose row.  cenv: the doubles the views Henv / Lenv hold.
//   an edge that names a row outside the graph, i == j, a point whose reference row is >= nkf or < -1     PSLFE_E_INVALID
//   an envelope above cenv doubles                                                                        PSLFE_E_CAPACITY
// Any number of keyframes may be fixed; an edge between two fixed ones enters the chi2 and nothing else.  Without a free
// keyframe or without an edge nothing is optimised (0 iterations) and the poses and points still come from the Sim3s given.
// A point with reference row -1 is copied.
template <class Exec>
PSL_EG_HD void psl_eg_run(Exec& X, const PslEgWs& W, int have, int code, size_t cenv, PslPose* pose_out, double* S_out, PslMapPointGeom* mp_out,
                          PslEgInfo* info) {
    int32_t* bad = W.flag + 1;
    if (have && code == PSLFE_OK) {
        X.one([&] { *bad = 0; });
        X.par(W.ne + W.nmp, [&](int t) {
            if (t < W.ne) {
                const PslEgEdge ed = W.ed[t];
                if (ed.i < 0 || ed.i >= W.nkf || ed.j < 0 || ed.j >= W.nkf || ed.i == ed.j) *bad = 1;
            } else if (W.mp_ref[t - W.ne] < -1 || W.mp_ref[t - W.ne] >= W.nkf) {
                *bad = 1;
            }
        });
        if (X.get(bad)) code = PSLFE_E_INVALID;
    }
    int F = 0;
    if (have && code == PSLFE_OK) {
        // the free indices; the items of every keyframe (a stable counting sort by keyframe: thread = keyframe, items in ascending order)
        X.par(W.nkf, [&](int v) {
            int n = 0;
            for (int e = 0; e < W.ne; ++e) n += (W.ed[e].i == v) + (W.ed[e].j == v);
            W.voff[v + 1] = n;
            psl_eg_load(W.kf[v].Scw, &W.S[v]);
            W.Sn[v] = W.S[v];
        });
        X.one([&] {
            int n = 0;
            W.voff[0] = 0;
            for (int v = 0; v < W.nkf; ++v) {
                W.voff[v + 1] += W.voff[v];
                W.pidx[v] = W.kf[v].fixed ? -1 : n;
                if (!W.kf[v].fixed) W.kfof[n++] = v;
            }
            W.flag[2] = n;
        });
        F = X.get(W.flag + 2);
        X.par(W.nkf, [&](int v) {
            int at = W.voff[v];
            for (int e = 0; e < W.ne; ++e) {
                if (W.ed[e].i == v) W.vlist[at++] = 2 * e;
                if (W.ed[e].j == v) W.vlist[at++] = 2 * e + 1;
            }
            psl_s3_inverse(&W.S[v], &W.Si[v]);
            W.Sni[v] = W.Si[v];
        });
        X.par(F, [&](int bi) {   // the envelope of block row bi
            const int v = W.kfof[bi];
            int lo = bi;
            for (int q = W.voff[v]; q < W.voff[v + 1]; ++q) {
                const int o = W.pidx[psl_eg_item_other(W, W.vlist[q])];
                if (o >= 0 && o < lo) lo = o;
            }
            W.fb[bi] = lo;
        });
        X.par(F, [&](int bj) {   // the last block row that reaches block column bj
            int bi = F - 1;
            while (bi > bj && W.fb[bi] > bj) --bi;
            W.lastblk[bj] = bi;
        });
        X.one([&] {
            int64_t off = 0;
            int over = 0;
            for (int r = 0; r < 7 * F; ++r) {
                const int64_t len = (int64_t)(r - 7 * W.fb[r / 7] + 1);
                if ((uint64_t)(off + len) > (uint64_t)cenv) { over = 1; break; }
                W.roff[r] = off;
                off += len;
            }
            W.flag[3] = over;
        });
        if (X.get(W.flag + 3)) code = PSLFE_E_CAPACITY;
    }
    if (!have || code != PSLFE_OK) {   // refused: the outputs are the inputs
        if (have) {
            X.par(W.nkf + W.nmp, [&](int t) {
                if (t < W.nkf) { for (int k = 0; k < 8; ++k) S_out[8 * (size_t)t + k] = W.kf[t].Scw[k]; }
                else { const PslMapPointGeom m = W.mp[t - W.nkf]; mp_out[t - W.nkf] = m; }
            });
        }
        X.one([&] {
            PslEgInfo I;
            I.status = code; I.iterations = 0; I.log_branches = 0; I.nfree = 0;
            I.chi2_start = 0.0; I.chi2_end = 0.0; I.lambda = 0.0;
            *info = I;
        });
        return;
    }
    double chi_first = 0.0, chi_last = 0.0, lambda = 0.0;
    int its = 0;
    if (F > 0 && W.ne > 0) {
        X.par(W.ne, [&](int e) { psl_eg_measure(W, e); });
        PslEgProblem P = {W, F, PSL_EG_LAMBDA_INIT};
        its = psl_lm_levenberg(X, P, PSL_EG_ITERATIONS, &chi_first, &chi_last, &lambda);
        X.one([&] {
            int m = 0;
            for (size_t t = 0; t < PSL_EG_EVALS * (size_t)W.ne; ++t) m |= W.bmask[t];
            W.flag[4] = m;
        });
    } else {
        X.one([&] { W.flag[4] = 0; });
    }
    const int mask = X.get(W.flag + 4);
    // the poses (src/Optimizer.cc:2747-2765): Sim3 [sR t; 0 1] -> SE3 [R t/s; 0 1]; vCorrectedSwc stays in Si for the points
    X.par(W.nkf, [&](int v) {
        const PslS3 S = W.S[v];
        psl_s3_inverse(&S, &W.Si[v]);
        double R[9];
        psl_po_quat_to_R(S.q, R);
        const double inv = PSL_LM_DIV(1.0, S.s);
        PslPose o;
        for (int k = 0; k < 9; ++k) o.R[k] = (float)R[k];
        for (int k = 0; k < 3; ++k) o.t[k] = (float)(S.t[k] * inv);
        pose_out[v] = o;
        psl_eg_store(&S, S_out + 8 * (size_t)v);
    });
    // the points (:2768-2798): correctedSwr.map(Srw.map(P)) with Srw the Sim3 the caller gave
    X.par(W.nmp, [&](int p) {
        PslMapPointGeom o = W.mp[p];
        const int r = W.mp_ref[p];
        if (r >= 0) {
            PslS3 Srw;
            psl_eg_load(W.kf[r].Scw, &Srw);
            const double P[3] = {(double)o.x, (double)o.y, (double)o.z};
            double a[3], c[3];
            psl_s3_map(&Srw, P, a);
            psl_s3_map(&W.Si[r], a, c);
            o.x = (float)c[0]; o.y = (float)c[1]; o.z = (float)c[2];
        }
        mp_out[p] = o;
    });
    X.one([&] {
        PslEgInfo I;
        I.status = PSLFE_OK; I.iterations = its; I.log_branches = mask; I.nfree = F;
        I.chi2_start = chi_first; I.chi2_end = chi_last; I.lambda = lambda;
        *info = I;
    });
}

#endif
