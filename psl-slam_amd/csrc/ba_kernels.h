// Optimizer::LocalBundleAdjustment and LocalBundleAdjustmentAndInseclines (pslfe_ba.hip): the point edges and, behind the drivers'
// compile-time switch LIL (as k_pose_optimize<true>), the VertexLIL vertices with their edges (the section before psl_ba_substitute;
// the LIL = false instantiations are the point-only text, unchanged).  The arithmetic of an edge, the quadratic form, the Schur
// complement, the dense LDLt solve in a run-time number of unknowns, g2o's Levenberg loop over many vertices and the two rounds
// with the decisions between them.  Product code.  Plain C++ text: k_ba_local includes it for the device and
// tools/dropin/ba_main.cpp for one core, so both run the same single IEEE operations (build with -ffp-contract=off; division and
// square root are PSL_LM_DIV / PSL_LM_SQRT, sin / cos the restated tables of psl_sincos_glibc.h, no device math library).
//
// One text for both.  Every step is a function of (workspace, index) that writes only what the index owns, and what runs the steps
// (psl_ba_solve, PslBaProblem, psl_ba_rounds) is a template over an executor `Exec`: par / one / sum256 / get, whose contract is in
// lm_kernels.h above psl_lm_levenberg.  PslLmSerial runs them on one core, PslLmWorkgroup of lm_device.h on the 256 threads of a
// workgroup.  Because no step depends on how its indices are spread, the two equal each other bit for bit by construction.
//
// The Levenberg loop - lambda, ni, the ten trials, rho, _nBad, Terminate, the failed solve - is the driver psl_lm_levenberg of
// lm_kernels.h; PslBaProblem gives it the steps over a system in HBM.  The loop has three texts that are changed together: the
// driver psl_lm_levenberg, and the two loops written out in k_pose_optimize and k_sim3_optimize.
//
// Restated from the reference:
//   EdgeSE3ProjectXYZ          Thirdparty/g2o/g2o/types/types_six_dof_expmap.h:90-106 (computeError, isDepthPositive), .cpp:103-148
//                              (linearizeOplus: _jacobianOplusXi w.r.t. the point, _jacobianOplusXj w.r.t. the pose; cam_project)
//   EdgeStereoSE3ProjectXYZ    .h:122-138, .cpp:150-236 (cam_project keeps its `const float invz`)
//   VertexSBAPointXYZ::oplusImpl   types_sba.h:52 (estimate += update); VertexSE3Expmap::oplusImpl types_six_dof_expmap.h:73
//                              (exp(update) * estimate)
//   constructQuadraticForm     core/base_binary_edge.hpp: with the robust kernel the weight rho[1] multiplies the information
//                              (rho[2] is not used); a fixed vertex gets no block and its edges contribute to the other vertex only
//   buildSystem, setLambda, restoreDiagonal, solve   core/block_solver.hpp:354-486, :502-603
//   Levenberg                  core/optimization_algorithm_levenberg.cpp:61-189
//   the two rounds             src/Optimizer.cc:1642-1790 (identical at :2356-2456)
// Pinned to g2o's text: the formulas of the errors and of both Jacobian halves as written there (x*y/z_2*fx is ((x*y)/z_2)*fx),
// lambda on the diagonal of EVERY pose and landmark block, Dinv = (Hll + lambda I)^-1 per landmark, db = Dinv bl,
// coefficients_i1 += B_i1 db, S_i1i2 -= (B_i1 Dinv) B_i2^T for i2 >= i1, bschur = bp - coefficients, cl = bl - B^T xp, xl = Dinv cl,
// computeLambdaInit and computeScale over the pose unknowns and then the landmark unknowns, the double chi2 against 5.991 / 7.815.
// This library's reading (Eigen is not in the reference tree): products of small matrices sum in index order, left to right; the
// 3x3 inverse is the closed form by cofactors times 1 / det; LinearSolverEigen (a sparse Cholesky behind a fill-reducing ordering)
// is the dense LDLt without pivoting of psl_lm_solve with a run-time N, in the caller's keyframe order, and a pivot that is not a
// finite positive number is "the solve failed"; a landmark whose Hll + lambda I has no finite inverse makes the trial a failed
// solve; a pose step that psl_lm_step_ok refuses likewise; a failed solve forms no candidate (lm_kernels.h).
// chi2() of an edge is g2o's cached _error: what the last computeActiveErrors left there - at the last candidate, accepted or
// not; an edge on level 1 keeps the error of round one.  isDepthPositive reads the estimates.
// The abort flag inside optimize() (pbStopFlag / forceStopFlag) is not modelled: a call runs to its end; `rounds = 1` is
// bDoMore == false.
//
// The order of every sum depends on nothing but the edge order and the counts.  A keyframe's Hpp block and bp take its edges in
// ascending edge index, a point's Hll and bl likewise; S_i1i2 and coefficients take the landmarks in ascending point row; cl takes
// a point's keyframes in ascending keyframe row (the rows of g2o's column-compressed Hpl).  No atomic floating-point add anywhere.
// Blocks follow the caller's row order: a caller who wants g2o's index mapping passes keyframes and points in ascending mnId.
#ifndef PSL_BA_KERNELS_H
#define PSL_BA_KERNELS_H

#include <stddef.h>

#include "../../include/pslfe.h"
#include "pose_kernels.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define PSL_BA_HD PSL_LM_HD
#define PSL_BA_ROW 28          // per edge: _jacobianOplusXj [3][6], _jacobianOplusXi [3][3], w = rho' * invSigma2
#define PSL_BA_LIL_ROW 55      // per LIL edge: _jacobianOplusXj [6][6], _jacobianOplusXi [6][3], w = rho' * 0.01
#define PSL_BA_LIL_INFO 0.01   // double invSigma = 0.01 (src/Optimizer.cc:1970): the information of a LIL edge is 0.01 * I6
#define PSL_BA_CHI2_LIL 11.07  // src/Optimizer.cc:2406, :2469
#define PSL_BA_CHI2_MONO 5.991
#define PSL_BA_CHI2_STEREO 7.815
#define PSL_GBA_DELTA_MONO 2.4474475383758545   /* thHuber2D = (float)sqrt(5.99) of Optimizer::BundleAdjustment (src/Optimizer.cc:85); its stereo delta is PSL_POSE_DELTA_STEREO */

// The workspace of one problem: views into one block of HBM (host: of one allocation), carved by psl_ba_carve.
struct PslBaWs {
    // the problem
    const PslBaKeyFrame* kf;
    const PslMapPointGeom* mp;
    const PslBaEdge* ed;
    int nkf, nmp, ne;
    PslPoseCamD K;
    const double* sctab;
    // estimates and candidates
    PslSE3 *T, *Tn;          // [nkf]
    double *X, *Xn;          // [nmp][3]
    // per edge
    double *err, *rho0, *row, *Hpl;   // [ne][3], [ne], [ne][28], [ne][18] (6 pose rows x 3 point columns)
    // the system: pose blocks by pose index i (0 <= i < F, the free keyframes with an active edge in row order)
    double *Hpp, *bp;        // [F][21] upper triangle row by row, [6 F]
    double *Hll, *bl, *Dinv, *db, *xl;   // [nmp][6] upper triangle, [nmp][3], [nmp][6], [nmp][3], [nmp][3]
    double *S, *Dd, *cc, *bs, *xp;       // [N][N] (upper: S, strictly lower: L), D [N], the hot column [N], bschur [N], x [N]
    double *scal;            // [8] values that every thread reads back; [8..263] the partial sums of the one-core sum256
    // the lists (stable counting sorts) and the bookkeeping of a round
    int32_t *koff, *poff;    // [nkf + 1], [nmp + 1]
    int32_t *klist, *plist, *kplist, *pklist;   // [ne]: by (keyframe, edge), (point, edge), (keyframe, point), (point, keyframe)
    int32_t *pidx, *kfof;    // [nkf] pose index of a keyframe or -1; [F] its inverse
    int32_t *cursor;         // [max(nkf, nmp) + 1]
    int32_t *flag;           // [4]
    uint8_t *level, *pact;   // [ne] 1: the edge is on level 1; [nmp] the point has an active edge
    // the VertexLIL vertices and their edges (the drivers' LIL = true instantiation only).  LIL j is landmark nmp + j: Hll, bl, Dinv,
    // db, xl and pact have nmp + nlil rows; LIL edge j has the global edge index ne + j
    const PslMapLil* lil = nullptr;
    const PslBaLilEdge* led = nullptr;
    int nlil = 0, nle = 0;
    double *L = nullptr, *Ln = nullptr;                                            // [nlil][15]
    double *lerr = nullptr, *lrho0 = nullptr, *lrow = nullptr, *lHpl = nullptr;    // [nle][6], [nle], [nle][55], [nle][18]
    int32_t *lkoff = nullptr, *lloff = nullptr;                                    // [nkf + 1], [nlil + 1]
    int32_t *lklist = nullptr, *lllist = nullptr, *lkllist = nullptr, *llklist = nullptr;   // [nle]: by (keyframe, edge), (LIL, edge), (keyframe, LIL), (LIL, keyframe)
    int32_t *lrank = nullptr, *larow = nullptr;   // [nlil] the rank i of an active LIL among the round's active LILs; its inverse a(i)
    uint8_t* llevel = nullptr;                    // [nle]
};

PSL_BA_HD size_t psl_ba_take(size_t* off, size_t bytes) {
    const size_t at = *off;
    *off = at + ((bytes + 7) & ~(size_t)7);
    return at;
}

// The views of a workspace for the caps (ckf, cmp, ced) and the LIL caps (clil, cle; negative: no LIL views) at base; returns its size in bytes (base may be NULL to ask for it).
PSL_BA_HD size_t psl_ba_carve(char* base, int ckf, int cmp, int ced, PslBaWs* W, int clil = -1, int cle = -1) {
    size_t off = 0;
    const size_t N = 6 * (size_t)ckf, D = sizeof(double), I = sizeof(int32_t);
    const int lils = clil >= 0 && cle >= 0;   // the LIL views, also for caps of 0: the LIL = true text reads their offsets
    if (!lils) { clil = 0; cle = 0; }
    const size_t cland = (size_t)cmp + (size_t)clil;
    const size_t cv = (size_t)(ckf > cmp ? (ckf > clil ? ckf : clil) : (cmp > clil ? cmp : clil)) + 1;
#define PSL_BA_VIEW(member, type, count) W->member = reinterpret_cast<type*>(base + psl_ba_take(&off, (count)))
    PSL_BA_VIEW(T, PslSE3, ckf * sizeof(PslSE3));
    PSL_BA_VIEW(Tn, PslSE3, ckf * sizeof(PslSE3));
    PSL_BA_VIEW(X, double, 3 * (size_t)cmp * D);
    PSL_BA_VIEW(Xn, double, 3 * (size_t)cmp * D);
    PSL_BA_VIEW(err, double, 3 * (size_t)ced * D);
    PSL_BA_VIEW(rho0, double, (size_t)ced * D);
    PSL_BA_VIEW(row, double, PSL_BA_ROW * (size_t)ced * D);
    PSL_BA_VIEW(Hpl, double, 18 * (size_t)ced * D);
    PSL_BA_VIEW(Hpp, double, 21 * (size_t)ckf * D);
    PSL_BA_VIEW(bp, double, N * D);
    PSL_BA_VIEW(Hll, double, 6 * cland * D);
    PSL_BA_VIEW(bl, double, 3 * cland * D);
    PSL_BA_VIEW(Dinv, double, 6 * cland * D);
    PSL_BA_VIEW(db, double, 3 * cland * D);
    PSL_BA_VIEW(xl, double, 3 * cland * D);
    PSL_BA_VIEW(S, double, N * N * D);
    PSL_BA_VIEW(Dd, double, N * D);
    PSL_BA_VIEW(cc, double, N * D);
    PSL_BA_VIEW(bs, double, N * D);
    PSL_BA_VIEW(xp, double, N * D);
    PSL_BA_VIEW(scal, double, (8 + PSL_LM_LANES) * D);
    PSL_BA_VIEW(koff, int32_t, ((size_t)ckf + 1) * I);
    PSL_BA_VIEW(poff, int32_t, ((size_t)cmp + 1) * I);
    PSL_BA_VIEW(klist, int32_t, (size_t)ced * I);
    PSL_BA_VIEW(plist, int32_t, (size_t)ced * I);
    PSL_BA_VIEW(kplist, int32_t, (size_t)ced * I);
    PSL_BA_VIEW(pklist, int32_t, (size_t)ced * I);
    PSL_BA_VIEW(pidx, int32_t, (size_t)ckf * I);
    PSL_BA_VIEW(kfof, int32_t, (size_t)ckf * I);
    PSL_BA_VIEW(cursor, int32_t, cv * I);
    PSL_BA_VIEW(flag, int32_t, 4 * I);
    PSL_BA_VIEW(level, uint8_t, (size_t)ced);
    PSL_BA_VIEW(pact, uint8_t, cland);
    if (lils) {
        PSL_BA_VIEW(L, double, 15 * (size_t)clil * D);
        PSL_BA_VIEW(Ln, double, 15 * (size_t)clil * D);
        PSL_BA_VIEW(lerr, double, 6 * (size_t)cle * D);
        PSL_BA_VIEW(lrho0, double, (size_t)cle * D);
        PSL_BA_VIEW(lrow, double, PSL_BA_LIL_ROW * (size_t)cle * D);
        PSL_BA_VIEW(lHpl, double, 18 * (size_t)cle * D);
        PSL_BA_VIEW(lkoff, int32_t, ((size_t)ckf + 1) * I);
        PSL_BA_VIEW(lloff, int32_t, ((size_t)clil + 1) * I);
        PSL_BA_VIEW(lklist, int32_t, (size_t)cle * I);
        PSL_BA_VIEW(lllist, int32_t, (size_t)cle * I);
        PSL_BA_VIEW(lkllist, int32_t, (size_t)cle * I);
        PSL_BA_VIEW(llklist, int32_t, (size_t)cle * I);
        PSL_BA_VIEW(lrank, int32_t, (size_t)clil * I);
        PSL_BA_VIEW(larow, int32_t, (size_t)clil * I);
        PSL_BA_VIEW(llevel, uint8_t, (size_t)cle);
    }
#undef PSL_BA_VIEW
    return off;
}

// the upper-triangle index of (j, k), j <= k, of an n x n matrix stored row by row
PSL_BA_HD int psl_ba_tri(int n, int j, int k) { return j * n - (j * (j - 1)) / 2 + (k - j); }
PSL_BA_HD int psl_ba_sym3(int j, int k) { return j <= k ? psl_ba_tri(3, j, k) : psl_ba_tri(3, k, j); }
PSL_BA_HD int psl_ba_finite(double v) { return __builtin_fabs(v) <= PSL_LM_DBL_MAX; }

// T.map(Xw) (se3quat.h: _r * xyz + _t)
PSL_BA_HD void psl_ba_map(const PslSE3* T, const double* Xw, double* Pc) {
    double r[3];
    psl_po_rotate(T->q, Xw, r);
    Pc[0] = r[0] + T->t[0]; Pc[1] = r[1] + T->t[1]; Pc[2] = r[2] + T->t[2];
}

// computeError of both edges (types_six_dof_expmap.h:96-101, :128-133) with cam_project (.cpp:141-157): e[2] = 0 for a monocular edge
PSL_BA_HD void psl_ba_error(const PslBaEdge* ed, const double* Pc, const PslPoseCamD* K, double* e) {
    if (ed->ur < 0.f) {
        e[0] = (double)ed->u - (PSL_LM_DIV(Pc[0], Pc[2]) * K->fx + K->cx);
        e[1] = (double)ed->v - (PSL_LM_DIV(Pc[1], Pc[2]) * K->fy + K->cy);
        e[2] = 0.0;
    } else {
        const double invz = (double)(float)PSL_LM_DIV(1.0, Pc[2]);
        const double r0 = (Pc[0] * invz) * K->fx + K->cx;
        e[0] = (double)ed->u - r0;
        e[1] = (double)ed->v - ((Pc[1] * invz) * K->fy + K->cy);
        e[2] = (double)ed->ur - (r0 - K->bf * invz);
    }
}

// linearizeOplus of both edges (types_six_dof_expmap.cpp:103-139, :188-234) at the camera point Pc and the rotation R of the pose:
// Jp = _jacobianOplusXj [3][6], Jl = _jacobianOplusXi [3][3]; row 2 is zero for a monocular edge.  The monocular point half is
// (-1./z * tmp) * R with every entry (a0 R0c + a1 R1c) + a2 R2c; the stereo one is written out entry by entry in g2o.
PSL_BA_HD void psl_ba_jacobians(int mono, const double* Pc, const double* R, const PslPoseCamD* K, double* Jp, double* Jl) {
    const double x = Pc[0], y = Pc[1], z = Pc[2], z_2 = z * z;
    const double fx = K->fx, fy = K->fy, bf = K->bf;
    Jp[0] = PSL_LM_DIV(x * y, z_2) * fx;
    Jp[1] = (-(1.0 + PSL_LM_DIV(x * x, z_2))) * fx;
    Jp[2] = PSL_LM_DIV(y, z) * fx;
    Jp[3] = PSL_LM_DIV(-1.0, z) * fx;
    Jp[4] = 0.0;
    Jp[5] = PSL_LM_DIV(x, z_2) * fx;
    Jp[6] = (1.0 + PSL_LM_DIV(y * y, z_2)) * fy;
    Jp[7] = PSL_LM_DIV((-x) * y, z_2) * fy;
    Jp[8] = PSL_LM_DIV(-x, z) * fy;
    Jp[9] = 0.0;
    Jp[10] = PSL_LM_DIV(-1.0, z) * fy;
    Jp[11] = PSL_LM_DIV(y, z_2) * fy;
    if (mono) {
        for (int k = 12; k < 18; ++k) Jp[k] = 0.0;
        const double m = PSL_LM_DIV(-1.0, z);
        const double a[6] = {m * fx, m * 0.0, m * (PSL_LM_DIV(-x, z) * fx), m * 0.0, m * fy, m * (PSL_LM_DIV(-y, z) * fy)};
        for (int i = 0; i < 2; ++i)
            for (int c = 0; c < 3; ++c) Jl[3 * i + c] = (a[3 * i] * R[c] + a[3 * i + 1] * R[3 + c]) + a[3 * i + 2] * R[6 + c];
        Jl[6] = 0.0; Jl[7] = 0.0; Jl[8] = 0.0;
    } else {
        Jp[12] = Jp[0] - PSL_LM_DIV(bf * y, z_2);
        Jp[13] = Jp[1] + PSL_LM_DIV(bf * x, z_2);
        Jp[14] = Jp[2];
        Jp[15] = Jp[3];
        Jp[16] = 0.0;
        Jp[17] = Jp[5] - PSL_LM_DIV(bf, z_2);
        for (int c = 0; c < 3; ++c) {
            Jl[c] = PSL_LM_DIV((-fx) * R[c], z) + PSL_LM_DIV((fx * x) * R[6 + c], z_2);
            Jl[3 + c] = PSL_LM_DIV((-fy) * R[3 + c], z) + PSL_LM_DIV((fy * y) * R[6 + c], z_2);
            Jl[6 + c] = Jl[c] - PSL_LM_DIV(bf * R[6 + c], z_2);
        }
    }
}

// computeActiveErrors of edge e at the estimates (Ts, Xs): its _error and the robust chi2; with `linearize` also linearizeOplus and
// the off-diagonal block Hpl of constructQuadraticForm, B[r][m] = (w Jp[0][r]) Jl[0][m] + (w Jp[1][r]) Jl[1][m] (+ row 2).
// GBA = true (gba_kernels.h): the Huber deltas of Optimizer::BundleAdjustment, whose monocular one is PSL_GBA_DELTA_MONO.
template <bool GBA = false>
PSL_BA_HD void psl_ba_edge(const PslBaWs& W, int e, const PslSE3* Ts, const double* Xs, int robust, int linearize) {
    if (W.level[e]) return;
    const PslBaEdge ed = W.ed[e];
    const PslSE3* T = Ts + ed.kf;
    const int mono = ed.ur < 0.f;
    double Pc[3], er[3];
    psl_ba_map(T, Xs + 3 * (size_t)ed.point, Pc);
    psl_ba_error(&ed, Pc, &W.K, er);
    const double is2 = (double)ed.inv_sigma2;
    const double c = psl_po_chi2(er, is2, mono);
    double rho0 = c, rho1 = 1.0;
    if (robust) psl_lm_huber(c, GBA && mono ? PSL_GBA_DELTA_MONO : PSL_POSE_DELTA(mono), &rho0, &rho1);
    W.err[3 * (size_t)e] = er[0]; W.err[3 * (size_t)e + 1] = er[1]; W.err[3 * (size_t)e + 2] = er[2];
    W.rho0[e] = rho0;
    if (!linearize) return;
    double* row = W.row + PSL_BA_ROW * (size_t)e;
    double R[9], Jp[18], Jl[9];
    psl_po_quat_to_R(T->q, R);
    psl_ba_jacobians(mono, Pc, R, &W.K, Jp, Jl);
    const double w = rho1 * is2;
    for (int k = 0; k < 18; ++k) row[k] = Jp[k];
    for (int k = 0; k < 9; ++k) row[18 + k] = Jl[k];
    row[27] = w;
    if (W.pidx[ed.kf] < 0) return;
    double* B = W.Hpl + 18 * (size_t)e;
    for (int r = 0; r < 6; ++r) {
        const double w0 = w * Jp[r], w1 = w * Jp[6 + r], w2 = w * Jp[12 + r];
        for (int m = 0; m < 3; ++m) {
            const double s = w0 * Jl[m] + w1 * Jl[3 + m];
            B[3 * r + m] = mono ? s : s + w2 * Jl[6 + m];
        }
    }
}

// One value of a vertex's diagonal block or of its b (constructQuadraticForm + copyB): n = 6 (a pose, J at row + 0) or 3 (a point,
// J at row + 18); h < n (n + 1) / 2: the upper-triangle entry h, else b[h - n (n + 1) / 2] with its sign.  The vertex's active
// edges in list order (ascending edge index).
PSL_BA_HD double psl_ba_block_sum(const PslBaWs& W, const int32_t* list, int i0, int i1, int n, int joff, int h) {
    const int nh = n * (n + 1) / 2;
    int j = 0, k = 0;
    if (h < nh) {
        int r = h;
        while (r >= n - j) { r -= n - j; ++j; }
        k = j + r;
    } else {
        j = h - nh;
    }
    double acc = 0.0;
    for (int a = i0; a < i1; ++a) {
        const int e = list[a];
        if (W.level[e]) continue;
        const double* row = W.row + PSL_BA_ROW * (size_t)e;
        const double* J = row + joff;
        const int mono = W.ed[e].ur < 0.f;
        const double w = row[27];
        const double w0 = w * J[j], w1 = w * J[n + j], w2 = w * J[2 * n + j];
        double s;
        if (h < nh) {
            s = w0 * J[k] + w1 * J[n + k];
            if (!mono) s = s + w2 * J[2 * n + k];
        } else {
            const double* er = W.err + 3 * (size_t)e;
            s = w0 * er[0] + w1 * er[1];
            if (!mono) s = s + w2 * er[2];
        }
        acc = acc + s;
    }
    return acc;
}
PSL_BA_HD double psl_ba_block_value(const PslBaWs& W, const int32_t* list, int i0, int i1, int n, int joff, int h) {
    const double acc = psl_ba_block_sum(W, list, i0, i1, n, joff, h);
    return h < n * (n + 1) / 2 ? acc : -acc;
}
PSL_BA_HD double psl_ba_lil_block_sum(const PslBaWs& W, const int32_t* list, int i0, int i1, int n, int joff, int h, double acc);
// with LIL: the keyframe's point-edge list and then its LIL-edge list as one running sum, in ascending global edge index
template <bool LIL>
PSL_BA_HD void psl_ba_build_pose(const PslBaWs& W, int t) {   // t < 27 F
    const int i = t / 27, h = t % 27, k = W.kfof[i];
    double v;
    if constexpr (LIL) {
        v = psl_ba_block_sum(W, W.klist, W.koff[k], W.koff[k + 1], 6, 0, h);
        v = psl_ba_lil_block_sum(W, W.lklist, W.lkoff[k], W.lkoff[k + 1], 6, 0, h, v);
        v = h < 21 ? v : -v;
    } else {
        v = psl_ba_block_value(W, W.klist, W.koff[k], W.koff[k + 1], 6, 0, h);
    }
    if (h < 21) W.Hpp[21 * (size_t)i + h] = v; else W.bp[6 * (size_t)i + (h - 21)] = v;
}
PSL_BA_HD void psl_ba_build_point(const PslBaWs& W, int t) {   // t < 9 nmp
    const int p = t / 9, h = t % 9;
    if (!W.pact[p]) return;
    const double v = psl_ba_block_value(W, W.plist, W.poff[p], W.poff[p + 1], 3, 18, h);
    if (h < 6) W.Hll[6 * (size_t)p + h] = v; else W.bl[3 * (size_t)p + (h - 6)] = v;
}

// the landmarks of the system: the points and, with LIL, the LILs after them
template <bool LIL>
PSL_BA_HD int psl_ba_nland(const PslBaWs& W) {
    if constexpr (LIL) return W.nmp + W.nlil; else return W.nmp;
}

// computeLambdaInit (optimization_algorithm_levenberg.cpp:166-180): tau * the largest |diagonal| over the pose blocks, then the
// landmark blocks, in index order
template <bool LIL>
PSL_BA_HD double psl_ba_lambda_init(const PslBaWs& W, int F) {
    double m = 0.0;
    for (int i = 0; i < F; ++i)
        for (int j = 0; j < 6; ++j) {
            const double a = __builtin_fabs(W.Hpp[21 * (size_t)i + psl_ba_tri(6, j, j)]);
            m = a < m ? m : a;
        }
    for (int p = 0; p < psl_ba_nland<LIL>(W); ++p) {
        if (!W.pact[p]) continue;
        for (int j = 0; j < 3; ++j) {
            const double a = __builtin_fabs(W.Hll[6 * (size_t)p + psl_ba_tri(3, j, j)]);
            m = a < m ? m : a;
        }
    }
    return 1e-5 * m;
}

// computeScale (:182-189): sum x_j (lambda x_j + b_j) over the pose unknowns, then the landmark unknowns, in index order
template <bool LIL>
PSL_BA_HD double psl_ba_scale(const PslBaWs& W, int F, double lambda) {
    double scale = 0.0;
    for (int j = 0; j < 6 * F; ++j) scale = scale + W.xp[j] * (lambda * W.xp[j] + W.bp[j]);
    for (int p = 0; p < psl_ba_nland<LIL>(W); ++p) {
        if (!W.pact[p]) continue;
        for (int j = 0; j < 3; ++j) {
            const double x = W.xl[3 * (size_t)p + j];
            scale = scale + x * (lambda * x + W.bl[3 * (size_t)p + j]);
        }
    }
    return scale;
}

// Dinv = (Hll + lambda I)^-1 of point p by cofactors, db = Dinv bl (block_solver.hpp:386-395); a non-finite entry clears *ok
PSL_BA_HD void psl_ba_point_inverse(const PslBaWs& W, int p, double lambda, int32_t* ok) {
    if (!W.pact[p]) return;
    const double* H = W.Hll + 6 * (size_t)p;
    const double a00 = H[0] + lambda, a01 = H[1], a02 = H[2], a11 = H[3] + lambda, a12 = H[4], a22 = H[5] + lambda;
    const double c00 = a11 * a22 - a12 * a12, c01 = a02 * a12 - a01 * a22, c02 = a01 * a12 - a02 * a11;
    const double c11 = a00 * a22 - a02 * a02, c12 = a01 * a02 - a00 * a12, c22 = a00 * a11 - a01 * a01;
    const double det = (a00 * c00 + a01 * c01) + a02 * c02;
    const double inv = PSL_LM_DIV(1.0, det);
    double* Di = W.Dinv + 6 * (size_t)p;
    Di[0] = c00 * inv; Di[1] = c01 * inv; Di[2] = c02 * inv; Di[3] = c11 * inv; Di[4] = c12 * inv; Di[5] = c22 * inv;
    int fin = 1;
    for (int k = 0; k < 6; ++k) fin &= psl_ba_finite(Di[k]);
    if (!fin) *ok = 0;
    const double* b = W.bl + 3 * (size_t)p;
    for (int j = 0; j < 3; ++j)
        W.db[3 * (size_t)p + j] = (Di[psl_ba_sym3(j, 0)] * b[0] + Di[psl_ba_sym3(j, 1)] * b[1]) + Di[psl_ba_sym3(j, 2)] * b[2];
}

// (B1 Dinv) B2^T at (r, c) for the landmark of the edges e1 (keyframe i1) and e2 (keyframe i2)
PSL_BA_HD double psl_ba_schur_term(const PslBaWs& W, int e1, int e2, int r, int c) {
    const double* B1 = W.Hpl + 18 * (size_t)e1 + 3 * r;
    const double* B2 = W.Hpl + 18 * (size_t)e2 + 3 * c;
    const double* Di = W.Dinv + 6 * (size_t)W.ed[e1].point;
    double BD[3];
    for (int k = 0; k < 3; ++k) BD[k] = (B1[0] * Di[psl_ba_sym3(0, k)] + B1[1] * Di[psl_ba_sym3(1, k)]) + B1[2] * Di[psl_ba_sym3(2, k)];
    return (BD[0] * B2[0] + BD[1] * B2[1]) + BD[2] * B2[2];
}

// One entry of the upper triangle of S = Hpp + lambda I - sum over the landmarks (block_solver.hpp:373-430): t < 36 F F names
// (i1, i2, r, c); entries below the diagonal are not formed.  The landmarks common to both keyframes in ascending point row: a
// merge of their (keyframe, point) lists.
PSL_BA_HD double psl_ba_lil_schur_sum(const PslBaWs& W, int k1, int k2, int r, int c, double s);
template <bool LIL>
PSL_BA_HD void psl_ba_schur_entry(const PslBaWs& W, int F, int t, double lambda) {
    const int blk = t / 36, r = (t % 36) / 6, c = t % 6;
    const int i1 = blk / F, i2 = blk % F;
    if (i2 < i1 || (i1 == i2 && c < r)) return;
    const int N = 6 * F;
    double s = 0.0;
    if (i1 == i2) {
        s = W.Hpp[21 * (size_t)i1 + psl_ba_tri(6, r, c)];
        if (r == c) s = s + lambda;
    }
    const int k1 = W.kfof[i1], k2 = W.kfof[i2];
    int a = W.koff[k1], b = W.koff[k2];
    const int a1 = W.koff[k1 + 1], b1 = W.koff[k2 + 1];
    while (a < a1 && b < b1) {
        const int ea = W.kplist[a], eb = W.kplist[b];
        const int pa = W.ed[ea].point, pb = W.ed[eb].point;
        if (pa < pb) { ++a; continue; }
        if (pb < pa) { ++b; continue; }
        if (!W.level[ea] && !W.level[eb]) s = s - psl_ba_schur_term(W, ea, eb, r, c);
        ++a; ++b;
    }
    if constexpr (LIL) s = psl_ba_lil_schur_sum(W, k1, k2, r, c, s);   // then the LILs in ascending row
    W.S[(size_t)(6 * i1 + r) * N + (6 * i2 + c)] = s;
}

// coefficients and bschur of pose unknown t < 6 F (block_solver.hpp:413, :436-439)
template <bool LIL>
PSL_BA_HD void psl_ba_bschur(const PslBaWs& W, int t) {
    const int i = t / 6, r = t % 6, k = W.kfof[i];
    double co = 0.0;
    for (int a = W.koff[k]; a < W.koff[k + 1]; ++a) {
        const int e = W.kplist[a];
        if (W.level[e]) continue;
        const double* B = W.Hpl + 18 * (size_t)e + 3 * r;
        const double* d = W.db + 3 * (size_t)W.ed[e].point;
        co = co + ((B[0] * d[0] + B[1] * d[1]) + B[2] * d[2]);
    }
    if constexpr (LIL)
        for (int a = W.lkoff[k]; a < W.lkoff[k + 1]; ++a) {
            const int e = W.lkllist[a];
            if (W.llevel[e]) continue;
            const double* B = W.lHpl + 18 * (size_t)e + 3 * r;
            const double* d = W.db + 3 * (size_t)(W.nmp + W.led[e].lil);
            co = co + ((B[0] * d[0] + B[1] * d[1]) + B[2] * d[2]);
        }
    W.bs[t] = W.bp[t] - co;
}

// cl = bl - B^T xp and xl = Dinv cl of point p (block_solver.hpp:461-481); a point's keyframes in ascending keyframe row
PSL_BA_HD void psl_ba_point_step(const PslBaWs& W, int p) {
    if (!W.pact[p]) return;
    double cl[3] = {W.bl[3 * (size_t)p], W.bl[3 * (size_t)p + 1], W.bl[3 * (size_t)p + 2]};
    for (int a = W.poff[p]; a < W.poff[p + 1]; ++a) {
        const int e = W.pklist[a];
        if (W.level[e]) continue;
        const int i = W.pidx[W.ed[e].kf];
        if (i < 0) continue;
        const double* B = W.Hpl + 18 * (size_t)e;
        const double* x = W.xp + 6 * (size_t)i;
        for (int j = 0; j < 3; ++j) {
            double s = B[j] * (-x[0]);
            for (int r = 1; r < 6; ++r) s = s + B[3 * r + j] * (-x[r]);
            cl[j] = cl[j] + s;
        }
    }
    const double* Di = W.Dinv + 6 * (size_t)p;
    for (int j = 0; j < 3; ++j)
        W.xl[3 * (size_t)p + j] = 0.0 + ((Di[psl_ba_sym3(j, 0)] * cl[0] + Di[psl_ba_sym3(j, 1)] * cl[1]) + Di[psl_ba_sym3(j, 2)] * cl[2]);
}

// ---- the VertexLIL vertices and the EdgeLILSE3ProjectXYZ edges of LocalBundleAdjustmentAndInseclines -------------------------------
// src/Optimizer.cc:2250-2533, add_inc/EdgeLIL.h:210-439, add_inc/VertexLIL.h.  A VertexLIL is a marginalised landmark of dimension
// 3 whose estimate has 15 doubles (line1 start / end, line2 start / end, crosspoint, :2277-2284); its id lies above every map point
// id, so the LILs follow the points in g2o's index mapping and LIL j is landmark nmp + j here.  One edge per (LIL, keyframe),
// created after all point edges (LIL edge j has the global edge index ne + j): measurement mvle_l[idx].first, .second,
// CrossPoint_2D[idx]; information 0.01 * I6 (`double invSigma = 0.01`, :1970); Huber with delta (float)sqrt(11.07).
// computeError, isDepthPositive and _jacobianOplusXj are the psl_po_lil_* functions of pose_kernels.h (row 2 of the Jacobian is
// evaluated at line 2's END point, EdgeLIL.h:273-275, so rows 2 and 3 of both halves are equal); _jacobianOplusXi (:315-337) is
// restated below.  The quadratic form is the point edges' reading with six rows: entry (j, k) of an edge is
// ((w J0j) J0k + (w J1j) J1k) + ... + (w J5j) J5k with w = rho' * 0.01.  chi2 is e0 (0.01 e0) + ... + e5 (0.01 e5).
// The levels (:2401-2414) and the erase flags (:2464-2478) are `chi2() > 11.07 || !isDepthPositive()` in double on the cached error.
//
// The update.  VertexLIL::oplusImpl (VertexLIL.h:23-27) maps FIFTEEN doubles at the update pointer and adds them to the estimate,
// but the vertex owns three of them: SparseOptimizer::update advances by dimension() = 3 (sparse_optimizer.cpp:425-434).  The next
// four 3-vectors of an active LIL therefore receive the steps of the next four active landmarks in g2o's order, and since the LILs
// come last those are the next four ACTIVE LILs.  For the last four active LILs the read runs past _xSize into the tail of _x, which
// Solver::resizeVector allocates (2 * sx, solver.cpp:51-54) and solve() never writes: zeros in a build without NDEBUG (:55-57) and
// whenever the allocation comes fresh from the kernel, indeterminate otherwise.
// This library's reading: a double past the end of the active update vector reads 0.0.  With a(0) < a(1) < ... the rows of the
// round's active LILs, Ln[a(i)][3 m + j] = L[a(i)][3 m + j] + (i + m < count ? xl[a(i + m)][j] : 0.0), m = 0 .. 4.  An inactive LIL
// is skipped as a follower and is itself not updated.  The reference's value is indeterminate at the last four active LILs, so parity
// there is unpinned even against a g2o build.
PSL_BA_HD double psl_ba_lil_chi2(const double* e) {
    double c = e[0] * (PSL_BA_LIL_INFO * e[0]);
    for (int r = 1; r < 6; ++r) c = c + e[r] * (PSL_BA_LIL_INFO * e[r]);
    return c;
}

// a line row of _jacobianOplusXi (EdgeLIL.h:315-329) at the camera point Pc with the line (l0, l1) and the rotation R:
// fx*l0*invz*R(0,c) + fy*l1*invz*R(1,c) - (fx*x*l0*invz_2 + fy*y*l1*invz_2)*R(2,c), every product left to right
PSL_BA_HD void psl_ba_lil_xi_line(const double* Pc, double l0, double l1, const double* R, const PslPoseCamD* K, double* J) {
    const double x = Pc[0], y = Pc[1], invz = PSL_LM_DIV(1.0, Pc[2]), invz2 = invz * invz;
    const double a = (K->fx * l0) * invz, b = (K->fy * l1) * invz;
    const double g = ((K->fx * x) * l0) * invz2 + ((K->fy * y) * l1) * invz2;
    for (int c = 0; c < 3; ++c) J[c] = (a * R[c] + b * R[3 + c]) - g * R[6 + c];
}
// rows 4 and 5 (:331-337) at the crosspoint, as written there: (4, 0) is -fx*invz*R(0,0) + fx*x*invz_2*R(2,0) while (4, 1) and (4, 2)
// are -fx*R(0,c)*invz + fx*x*R(2,c)*invz_2; row 5 is -fy*invz*R(1,c) + fy*y*invz_2*R(2,c) throughout
PSL_BA_HD void psl_ba_lil_xi_ins(const double* Pc, const double* R, const PslPoseCamD* K, double* J4, double* J5) {
    const double x = Pc[0], y = Pc[1], invz = PSL_LM_DIV(1.0, Pc[2]), invz2 = invz * invz;
    const double fx = K->fx, fy = K->fy;
    J4[0] = ((-fx) * invz) * R[0] + ((fx * x) * invz2) * R[6];
    J4[1] = ((-fx) * R[1]) * invz + ((fx * x) * R[7]) * invz2;
    J4[2] = ((-fx) * R[2]) * invz + ((fx * x) * R[8]) * invz2;
    for (int c = 0; c < 3; ++c) J5[c] = ((-fy) * invz) * R[3 + c] + ((fy * y) * invz2) * R[6 + c];
}

// computeActiveErrors of LIL edge e at the estimates (Ts, Ls), as psl_ba_edge: with `linearize` the row (Jp [6][6] at 0, Jl [6][3] at
// 36, w at 54) and the block Hpl, B[r][m] = ((w Jp[0][r]) Jl[0][m] + (w Jp[1][r]) Jl[1][m]) + ... + (w Jp[5][r]) Jl[5][m]
PSL_BA_HD void psl_ba_lil_edge(const PslBaWs& W, int e, const PslSE3* Ts, const double* Ls, int robust, int linearize) {
    if (W.llevel[e]) return;
    const PslBaLilEdge ed = W.led[e];
    const PslSE3* T = Ts + ed.kf;
    double Lr[PSL_POSE_LIL_DOUBLES], er[6];
    for (int k = 0; k < 15; ++k) Lr[k] = Ls[15 * (size_t)ed.lil + k];
    for (int k = 0; k < 3; ++k) { Lr[15 + k] = ed.obs1[k]; Lr[18 + k] = ed.obs2[k]; }
    Lr[21] = ed.obs_ins[0]; Lr[22] = ed.obs_ins[1];
    psl_po_lil_error(Lr, T, &W.K, er);
    const double c = psl_ba_lil_chi2(er);
    double rho0 = c, rho1 = 1.0;
    if (robust) psl_lm_huber(c, PSL_POSE_DELTA_LIL, &rho0, &rho1);
    for (int r = 0; r < 6; ++r) W.lerr[6 * (size_t)e + r] = er[r];
    W.lrho0[e] = rho0;
    if (!linearize) return;
    double* row = W.lrow + PSL_BA_LIL_ROW * (size_t)e;
    double R[9], Pc[3];
    psl_po_quat_to_R(T->q, R);
    for (int r = 0; r < 4; ++r) {
        const double* l = Lr + 15 + 3 * (r >> 1);
        psl_po_lil_map(Lr + (r == 2 ? 9 : 3 * r), T, Pc);   // EdgeLIL.h:273-275: segment<3>(9) twice
        psl_po_lil_row_line(Pc, l[0], l[1], &W.K, row + 6 * r);
        psl_ba_lil_xi_line(Pc, l[0], l[1], R, &W.K, row + 36 + 3 * r);
    }
    psl_po_lil_map(Lr + 12, T, Pc);
    psl_po_lil_row_ins(Pc, 0, &W.K, row + 24);
    psl_po_lil_row_ins(Pc, 1, &W.K, row + 30);
    psl_ba_lil_xi_ins(Pc, R, &W.K, row + 48, row + 51);
    const double w = rho1 * PSL_BA_LIL_INFO;
    row[54] = w;
    if (W.pidx[ed.kf] < 0) return;
    double* B = W.lHpl + 18 * (size_t)e;
    for (int r = 0; r < 6; ++r)
        for (int m = 0; m < 3; ++m) {
            double s = (w * row[r]) * row[36 + m];
            for (int a = 1; a < 6; ++a) s = s + (w * row[6 * a + r]) * row[36 + 3 * a + m];
            B[3 * r + m] = s;
        }
}

// psl_ba_block_sum over a list of LIL edges, continuing the running sum acc: n = 6 (J at row + 0) or 3 (J at row + 36)
PSL_BA_HD double psl_ba_lil_block_sum(const PslBaWs& W, const int32_t* list, int i0, int i1, int n, int joff, int h, double acc) {
    const int nh = n * (n + 1) / 2;
    int j = 0, k = 0;
    if (h < nh) {
        int r = h;
        while (r >= n - j) { r -= n - j; ++j; }
        k = j + r;
    } else {
        j = h - nh;
    }
    for (int a = i0; a < i1; ++a) {
        const int e = list[a];
        if (W.llevel[e]) continue;
        const double* row = W.lrow + PSL_BA_LIL_ROW * (size_t)e;
        const double* J = row + joff;
        const double* er = W.lerr + 6 * (size_t)e;
        const double w = row[54];
        double s = (w * J[j]) * (h < nh ? J[k] : er[0]);
        for (int r = 1; r < 6; ++r) s = s + (w * J[r * n + j]) * (h < nh ? J[r * n + k] : er[r]);
        acc = acc + s;
    }
    return acc;
}
PSL_BA_HD void psl_ba_build_lil(const PslBaWs& W, int t) {   // t < 9 nlil
    const int j = t / 9, h = t % 9, p = W.nmp + j;
    if (!W.pact[p]) return;
    const double v = psl_ba_lil_block_sum(W, W.lllist, W.lloff[j], W.lloff[j + 1], 3, 36, h, 0.0);
    if (h < 6) W.Hll[6 * (size_t)p + h] = v; else W.bl[3 * (size_t)p + (h - 6)] = -v;
}

// the LIL part of psl_ba_schur_entry: the LILs common to the keyframes k1 and k2 in ascending LIL row
PSL_BA_HD double psl_ba_lil_schur_sum(const PslBaWs& W, int k1, int k2, int r, int c, double s) {
    int a = W.lkoff[k1], b = W.lkoff[k2];
    const int a1 = W.lkoff[k1 + 1], b1 = W.lkoff[k2 + 1];
    while (a < a1 && b < b1) {
        const int ea = W.lkllist[a], eb = W.lkllist[b];
        const int pa = W.led[ea].lil, pb = W.led[eb].lil;
        if (pa < pb) { ++a; continue; }
        if (pb < pa) { ++b; continue; }
        if (!W.llevel[ea] && !W.llevel[eb]) {
            const double* B1 = W.lHpl + 18 * (size_t)ea + 3 * r;
            const double* B2 = W.lHpl + 18 * (size_t)eb + 3 * c;
            const double* Di = W.Dinv + 6 * (size_t)(W.nmp + pa);
            double BD[3];
            for (int k = 0; k < 3; ++k) BD[k] = (B1[0] * Di[psl_ba_sym3(0, k)] + B1[1] * Di[psl_ba_sym3(1, k)]) + B1[2] * Di[psl_ba_sym3(2, k)];
            s = s - ((BD[0] * B2[0] + BD[1] * B2[1]) + BD[2] * B2[2]);
        }
        ++a; ++b;
    }
    return s;
}

// psl_ba_point_step of LIL j: its keyframes in ascending keyframe row
PSL_BA_HD void psl_ba_lil_step(const PslBaWs& W, int j) {
    const int p = W.nmp + j;
    if (!W.pact[p]) return;
    double cl[3] = {W.bl[3 * (size_t)p], W.bl[3 * (size_t)p + 1], W.bl[3 * (size_t)p + 2]};
    for (int a = W.lloff[j]; a < W.lloff[j + 1]; ++a) {
        const int e = W.llklist[a];
        if (W.llevel[e]) continue;
        const int i = W.pidx[W.led[e].kf];
        if (i < 0) continue;
        const double* B = W.lHpl + 18 * (size_t)e;
        const double* x = W.xp + 6 * (size_t)i;
        for (int m = 0; m < 3; ++m) {
            double s = B[m] * (-x[0]);
            for (int r = 1; r < 6; ++r) s = s + B[3 * r + m] * (-x[r]);
            cl[m] = cl[m] + s;
        }
    }
    const double* Di = W.Dinv + 6 * (size_t)p;
    for (int m = 0; m < 3; ++m)
        W.xl[3 * (size_t)p + m] = 0.0 + ((Di[psl_ba_sym3(m, 0)] * cl[0] + Di[psl_ba_sym3(m, 1)] * cl[1]) + Di[psl_ba_sym3(m, 2)] * cl[2]);
}

// VertexLIL::oplusImpl of LIL j under the header's reading: `count` active LILs this round, ranked by W.lrank / W.larow
PSL_BA_HD void psl_ba_lil_update(const PslBaWs& W, int j, int count) {
    if (!W.pact[W.nmp + j]) return;
    const int i = W.lrank[j];
    for (int m = 0; m < 5; ++m)
        for (int c = 0; c < 3; ++c) {
            const double step = i + m < count ? W.xl[3 * (size_t)(W.nmp + W.larow[i + m]) + c] : 0.0;
            W.Ln[15 * (size_t)j + 3 * m + c] = W.L[15 * (size_t)j + 3 * m + c] + step;
        }
}

// `bad` of LIL edge e after a round (src/Optimizer.cc:2406, :2469): chi2() > 11.07 || !isDepthPositive(), in double
PSL_BA_HD int psl_ba_lil_edge_bad(const PslBaWs& W, int e) {
    const PslBaLilEdge ed = W.led[e];
    const double c = psl_ba_lil_chi2(W.lerr + 6 * (size_t)e);
    int positive = 1;
    for (int m = 0; m < 5; ++m) {
        double Pc[3];
        psl_po_lil_map(W.L + 15 * (size_t)ed.lil + 3 * m, W.T + ed.kf, Pc);
        positive &= Pc[2] > 0.0;
    }
    return (c > PSL_BA_CHI2_LIL) || !positive;
}

// the two substitutions of psl_lm_solve with a run-time N, on one thread: L y = bs, then x = D^-1 y - L^T x
PSL_BA_HD void psl_ba_substitute(const PslBaWs& W, int N) {
    double* y = W.cc;
    for (int i = 0; i < N; ++i) {
        double s = W.bs[i];
        for (int k = 0; k < i; ++k) s = s - W.S[(size_t)i * N + k] * y[k];
        y[i] = s;
    }
    for (int i = N - 1; i >= 0; --i) {
        double s = PSL_LM_DIV(y[i], W.Dd[i]);
        for (int k = i + 1; k < N; ++k) s = s - W.S[(size_t)k * N + i] * W.xp[k];
        W.xp[i] = s;
    }
}

// BlockSolver::solve at `lambda` (setLambda ... restoreDiagonal around it): 1 and xp, xl, or 0, "the solve failed".
// The LDLt of S is psl_lm_solve's with a run-time N, a column at a time: c[k] = L[j][k] D[k] for the column's row j, then every row
// i >= j forms d = A[j][j] - sum_k L[j][k] c[k] in ascending k (row j keeps it as D[j]) and L[i][j] = (A[i][j] - sum_k L[i][k] c[k]) / d.
// A[i][j] with i > j is read from the upper triangle at [j][i]; L overwrites the strictly lower one.
template <bool LIL, class Exec>
PSL_BA_HD int psl_ba_solve(Exec& X, const PslBaWs& W, int F, double lambda) {
    const int N = 6 * F;
    int32_t* ok = W.flag;
    X.one([&] { *ok = 1; });
    X.par(psl_ba_nland<LIL>(W), [&](int p) { psl_ba_point_inverse(W, p, lambda, ok); });
    if (!X.get(ok)) return 0;
    X.par(36 * F * F, [&](int t) { psl_ba_schur_entry<LIL>(W, F, t, lambda); });
    X.par(N, [&](int t) { psl_ba_bschur<LIL>(W, t); });
    for (int j = 0; j < N; ++j) {
        X.par(j, [&](int k) { W.cc[k] = W.S[(size_t)j * N + k] * W.Dd[k]; });
        X.par(N - j, [&](int t) {
            const int i = j + t;
            double d = W.S[(size_t)j * N + j];
            for (int k = 0; k < j; ++k) d = d - W.S[(size_t)j * N + k] * W.cc[k];
            if (i == j) {
                if (!(d > 0.0) || !(d <= PSL_LM_DBL_MAX)) *ok = 0;
                W.Dd[j] = d;
                return;
            }
            double s = W.S[(size_t)j * N + i];
            for (int k = 0; k < j; ++k) s = s - W.S[(size_t)i * N + k] * W.cc[k];
            W.S[(size_t)i * N + j] = PSL_LM_DIV(s, d);
        });
    }
    if (!X.get(ok)) return 0;
    X.one([&] { psl_ba_substitute(W, N); });
    X.par(F, [&](int i) { if (!psl_lm_step_ok(W.xp + 6 * (size_t)i)) *ok = 0; });
    if (!X.get(ok)) return 0;
    X.par(W.nmp, [&](int p) { psl_ba_point_step(W, p); });
    if constexpr (LIL) X.par(W.nlil, [&](int j) { psl_ba_lil_step(W, j); });
    return 1;
}

// the partial sum p of 256 of the robust chi2: the active edges p, p + 256, ... in ascending order
// (with LIL over the global edge index: the point edges 0 .. ne, then LIL edge j at ne + j)
template <bool LIL>
PSL_BA_HD double psl_ba_chi_partial(const PslBaWs& W, int p) {
    double s = 0.0;
    int e = p;
    for (; e < W.ne; e += PSL_LM_LANES)
        if (!W.level[e]) s = s + W.rho0[e];
    if constexpr (LIL)
        for (e -= W.ne; e < W.nle; e += PSL_LM_LANES)
            if (!W.llevel[e]) s = s + W.lrho0[e];
    return s;
}

// The `Problem` of psl_lm_levenberg (lm_kernels.h) for one optimize() call over the F pose blocks and the active points.
// With LIL the LIL edges are evaluated in a step of their own, and `nact` is the number of active LILs of the round.
template <bool LIL>
struct PslBaProblem {
    const PslBaWs& W;
    int F, nact, robust;
    template <class Exec> PSL_LM_MEMBER double linearize(Exec& X, double* chi_first) {
        X.par(W.ne, [&](int e) { psl_ba_edge(W, e, W.T, W.X, robust, 1); });
        if constexpr (LIL) X.par(W.nle, [&](int e) { psl_ba_lil_edge(W, e, W.T, W.L, robust, 1); });
        const double chi = X.sum256([&](int p) { return psl_ba_chi_partial<LIL>(W, p); });
        if (chi_first) *chi_first = chi;
        X.par(27 * F, [&](int t) { psl_ba_build_pose<LIL>(W, t); });
        X.par(9 * W.nmp, [&](int t) { psl_ba_build_point(W, t); });
        if constexpr (LIL) X.par(9 * W.nlil, [&](int t) { psl_ba_build_lil(W, t); });
        return chi;
    }
    template <class Exec> PSL_LM_MEMBER double lambda_init(Exec& X) {
        X.one([&] { W.scal[0] = psl_ba_lambda_init<LIL>(W, F); });
        return X.get(W.scal);
    }
    template <class Exec> PSL_LM_MEMBER int solve(Exec& X, double lambda) { return psl_ba_solve<LIL>(X, W, F, lambda); }
    template <class Exec> PSL_LM_MEMBER double candidate(Exec& X) {
        X.par(W.nkf + W.nmp, [&](int v) {   // oplusImpl of every active vertex
            if (v < W.nkf) {
                const int i = W.pidx[v];
                if (i < 0) return;
                PslSE3 dT;
                psl_po_exp(W.xp + 6 * (size_t)i, &dT, W.sctab);
                psl_po_mul(&dT, &W.T[v], &W.Tn[v]);
            } else {
                const int p = v - W.nkf;
                if (!W.pact[p]) return;
                for (int j = 0; j < 3; ++j) W.Xn[3 * (size_t)p + j] = W.X[3 * (size_t)p + j] + W.xl[3 * (size_t)p + j];
            }
        });
        if constexpr (LIL) X.par(W.nlil, [&](int j) { psl_ba_lil_update(W, j, nact); });
        X.par(W.ne, [&](int e) { psl_ba_edge(W, e, W.Tn, W.Xn, robust, 0); });
        if constexpr (LIL) X.par(W.nle, [&](int e) { psl_ba_lil_edge(W, e, W.Tn, W.Ln, robust, 0); });
        return X.sum256([&](int p) { return psl_ba_chi_partial<LIL>(W, p); });
    }
    template <class Exec> PSL_LM_MEMBER double scale(Exec& X, double lambda) {
        X.one([&] { W.scal[1] = psl_ba_scale<LIL>(W, F, lambda); });
        return X.get(W.scal + 1);
    }
    template <class Exec> PSL_LM_MEMBER void accept(Exec& X) {   // discardTop: the candidate becomes the estimate
        if constexpr (LIL)
            X.par(15 * W.nlil, [&](int t) {
                if (W.pact[W.nmp + t / 15]) W.L[t] = W.Ln[t];
            });
        X.par(W.nkf + W.nmp, [&](int v) {
            if (v < W.nkf) {
                if (W.pidx[v] >= 0) W.T[v] = W.Tn[v];
            } else {
                const int p = v - W.nkf;
                if (!W.pact[p]) return;
                for (int j = 0; j < 3; ++j) W.X[3 * (size_t)p + j] = W.Xn[3 * (size_t)p + j];
            }
        });
    }
};

// `bad` of edge e after a round (src/Optimizer.cc:1663, :1679, :1755, :1770): the plain chi2 of its cached _error as a double
// against 5.991 / 7.815, or !isDepthPositive at the estimates
PSL_BA_HD int psl_ba_edge_bad(const PslBaWs& W, int e) {
    const PslBaEdge ed = W.ed[e];
    const int mono = ed.ur < 0.f;
    const double c = psl_po_chi2(W.err + 3 * (size_t)e, (double)ed.inv_sigma2, mono);
    double Pc[3];
    psl_ba_map(W.T + ed.kf, W.X + 3 * (size_t)ed.point, Pc);
    return (c > (mono ? PSL_BA_CHI2_MONO : PSL_BA_CHI2_STEREO)) || !(Pc[2] > 0.0);
}

// The whole of LocalBundleAdjustment's optimisation on a checked problem whose lists are built: the estimates from the rows
// (toSE3Quat, toVector3d), round one optimize(5) with Huber on every edge, the levels, round two initializeOptimization(0) and
// optimize(10) without the kernel (rounds == 2), the erase flags, the rows out (toCvMat).  A vertex without an active edge is not
// in the system of a round; a round without a free keyframe in its system runs no iteration but still evaluates the active errors
// (g2o is never called that way).  kf_out / mp_out may be the input rows.  `info` is written by one().
// With LIL: the 15 doubles of every LIL come back in lil_out (:2526-2531; a LIL without an edge is not in the system and is
// copied), erase_lil gets the LIL edges' flags and *nerased_lil (may be NULL) their count; info->nerased counts point edges.
template <bool LIL = false, class Exec>
PSL_BA_HD void psl_ba_rounds(Exec& X, const PslBaWs& W, int rounds, PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out, uint8_t* erase,
                             PslBaInfo* info, PslMapLil* lil_out = nullptr, uint8_t* erase_lil = nullptr, int32_t* nerased_lil = nullptr) {
    X.par(W.nkf + W.nmp + W.ne, [&](int v) {
        if (v < W.nkf) {
            psl_po_from_pose(W.kf[v].Tcw.R, W.kf[v].Tcw.t, &W.T[v]);
            W.Tn[v] = W.T[v];
        } else if (v < W.nkf + W.nmp) {
            const int p = v - W.nkf;
            const double x[3] = {(double)W.mp[p].x, (double)W.mp[p].y, (double)W.mp[p].z};
            for (int j = 0; j < 3; ++j) { W.X[3 * (size_t)p + j] = x[j]; W.Xn[3 * (size_t)p + j] = x[j]; }
        } else {
            const int e = v - W.nkf - W.nmp;
            W.level[e] = 0;
            W.err[3 * (size_t)e] = 0.0; W.err[3 * (size_t)e + 1] = 0.0; W.err[3 * (size_t)e + 2] = 0.0;
            W.rho0[e] = 0.0;
        }
    });
    if constexpr (LIL)
        X.par(W.nlil + W.nle, [&](int v) {
            if (v < W.nlil) {
                for (int k = 0; k < 15; ++k) { const double x = W.lil[v].w[k]; W.L[15 * (size_t)v + k] = x; W.Ln[15 * (size_t)v + k] = x; }
            } else {
                const int e = v - W.nlil;
                W.llevel[e] = 0;
                for (int r = 0; r < 6; ++r) W.lerr[6 * (size_t)e + r] = 0.0;
                W.lrho0[e] = 0.0;
            }
        });
    double chi_start = 0.0, chi_r[2] = {0.0, 0.0};
    int its[2] = {0, 0};
    for (int r = 0; r < rounds; ++r) {
        const int robust = r == 0;
        X.par(W.nkf + W.nmp, [&](int v) {   // initializeOptimization(0): the vertices with an edge on level 0
            const int32_t* list = v < W.nkf ? W.klist : W.plist;
            const int32_t* off = v < W.nkf ? W.koff + v : W.poff + (v - W.nkf);
            int any = 0;
            for (int a = off[0]; a < off[1]; ++a) any |= !W.level[list[a]];
            if constexpr (LIL)
                if (v < W.nkf)
                    for (int a = W.lkoff[v]; a < W.lkoff[v + 1]; ++a) any |= !W.llevel[W.lklist[a]];
            if (v < W.nkf) W.pidx[v] = any && !W.kf[v].fixed ? 0 : -1; else W.pact[v - W.nkf] = (uint8_t)any;
        });
        X.one([&] {
            int F = 0;
            for (int k = 0; k < W.nkf; ++k)
                if (W.pidx[k] >= 0) { W.pidx[k] = F; W.kfof[F] = k; ++F; }
            W.flag[1] = F;
        });
        int nact = 0;
        if constexpr (LIL) {
            X.par(W.nlil, [&](int j) {
                int any = 0;
                for (int a = W.lloff[j]; a < W.lloff[j + 1]; ++a) any |= !W.llevel[W.lllist[a]];
                W.pact[W.nmp + j] = (uint8_t)any;
            });
            X.one([&] {   // the rank of the active LILs: a prefix count in row order
                int n = 0;
                for (int j = 0; j < W.nlil; ++j)
                    if (W.pact[W.nmp + j]) { W.lrank[j] = n; W.larow[n] = j; ++n; }
                W.flag[2] = n;
            });
            nact = X.get(W.flag + 2);
        }
        const int F = X.get(W.flag + 1);
        double first = 0.0, last = r ? chi_r[0] : 0.0;
        if (F > 0) {
            PslBaProblem<LIL> P = {W, F, nact, robust};
            double lambda;
            its[r] = psl_lm_levenberg(X, P, r == 0 ? 5 : 10, &first, &last, &lambda);
        } else {
            X.par(W.ne, [&](int e) { psl_ba_edge(W, e, W.T, W.X, robust, 0); });
            if constexpr (LIL) X.par(W.nle, [&](int e) { psl_ba_lil_edge(W, e, W.T, W.L, robust, 0); });
            first = last = X.sum256([&](int p) { return psl_ba_chi_partial<LIL>(W, p); });
        }
        if (r == 0) chi_start = first;
        chi_r[r] = last;
        const int final_round = r + 1 == rounds;
        X.par(W.ne, [&](int e) {
            const int bad = psl_ba_edge_bad(W, e);
            if (final_round) erase[e] = (uint8_t)bad; else W.level[e] = (uint8_t)bad;   // setLevel(1); setRobustKernel(0) is `robust`
        });
        if constexpr (LIL)
            X.par(W.nle, [&](int e) {
                const int bad = psl_ba_lil_edge_bad(W, e);
                if (final_round) erase_lil[e] = (uint8_t)bad; else W.llevel[e] = (uint8_t)bad;
            });
    }
    const double ner = X.sum256([&](int p) {   // a count: exact in any order
        double s = 0.0;
        for (int e = p; e < W.ne; e += PSL_LM_LANES) s = s + (erase[e] ? 1.0 : 0.0);
        return s;
    });
    if constexpr (LIL) {
        const double nel = X.sum256([&](int p) {
            double s = 0.0;
            for (int e = p; e < W.nle; e += PSL_LM_LANES) s = s + (erase_lil[e] ? 1.0 : 0.0);
            return s;
        });
        X.par(W.nlil, [&](int j) {
            PslMapLil o = W.lil[j];
            for (int k = 0; k < 15; ++k) o.w[k] = W.L[15 * (size_t)j + k];
            lil_out[j] = o;
        });
        X.one([&] { if (nerased_lil) *nerased_lil = (int32_t)nel; });
    }
    X.par(W.nkf + W.nmp, [&](int v) {
        if (v < W.nkf) {
            PslBaKeyFrame o = W.kf[v];
            if (!o.fixed) psl_po_to_pose(&W.T[v], o.Tcw.R, o.Tcw.t);   // SetPose of every local keyframe; a fixed camera is not written
            kf_out[v] = o;
        } else {
            const int p = v - W.nkf;
            PslMapPointGeom o = W.mp[p];
            o.x = (float)W.X[3 * (size_t)p]; o.y = (float)W.X[3 * (size_t)p + 1]; o.z = (float)W.X[3 * (size_t)p + 2];
            mp_out[p] = o;
        }
    });
    X.one([&] {
        PslBaInfo I;
        I.status = PSLFE_OK; I.rounds = rounds; I.iterations[0] = its[0]; I.iterations[1] = its[1]; I.nerased = (int32_t)ner;
        I.chi2_start = chi_start; I.chi2_round1 = chi_r[0]; I.chi2_end = chi_r[rounds - 1];
        *info = I;
    });
}

// ---- the checks and the lists on one core (the device forms: k_ba_check and k_ba_lists of pslfe_ba.hip) -----------------------------
// PSLFE_OK, or PSLFE_E_INVALID for an edge that names a row outside the problem.  (Capacity is the handle's matter.)
PSL_LM_HD int psl_ba_check_rows(const PslBaEdge* ed, int nkf, int nmp, int ne) {
    for (int e = 0; e < ne; ++e)
        if (ed[e].kf < 0 || ed[e].kf >= nkf || ed[e].point < 0 || ed[e].point >= nmp) return PSLFE_E_INVALID;
    return PSLFE_OK;
}
PSL_LM_HD int psl_ba_check_lil_rows(const PslBaLilEdge* led, int nkf, int nlil, int nle) {
    for (int e = 0; e < nle; ++e)
        if (led[e].kf < 0 || led[e].kf >= nkf || led[e].lil < 0 || led[e].lil >= nlil) return PSLFE_E_INVALID;
    return PSLFE_OK;
}
// 1 when the problem has something to optimise: an edge (of either kind: ne counts both) and a free keyframe
PSL_LM_HD int psl_ba_has_work(const PslBaKeyFrame* kf, int nkf, int ne) {
    int nfree = 0;
    for (int k = 0; k < nkf; ++k) nfree += !kf[k].fixed;
    return ne > 0 && nfree > 0;
}

#if !defined(__HIP_DEVICE_COMPILE__)
// a stable counting sort of the edges src[0..ne) (NULL: 0, 1, 2, ...) by key (0: keyframe, 1: point) into dst; off [nkeys + 1]
static inline void psl_ba_sort_host(const PslBaEdge* ed, int ne, const int32_t* src, int by_point, int nkeys, int32_t* off, int32_t* cursor,
                                    int32_t* dst) {
    for (int k = 0; k <= nkeys; ++k) off[k] = 0;
    for (int e = 0; e < ne; ++e) ++off[(by_point ? ed[e].point : ed[e].kf) + 1];
    for (int k = 0; k < nkeys; ++k) off[k + 1] += off[k];
    for (int k = 0; k < nkeys; ++k) cursor[k] = off[k];
    for (int a = 0; a < ne; ++a) {
        const int e = src ? src[a] : a;
        dst[cursor[by_point ? ed[e].point : ed[e].kf]++] = e;
    }
}
// the four lists of a checked problem; PSLFE_E_INVALID for a duplicate (point, keyframe) pair
static inline int psl_ba_lists_host(const PslBaWs& W) {
    psl_ba_sort_host(W.ed, W.ne, nullptr, 0, W.nkf, W.koff, W.cursor, W.klist);
    psl_ba_sort_host(W.ed, W.ne, nullptr, 1, W.nmp, W.poff, W.cursor, W.plist);
    psl_ba_sort_host(W.ed, W.ne, W.plist, 0, W.nkf, W.koff, W.cursor, W.kplist);
    psl_ba_sort_host(W.ed, W.ne, W.klist, 1, W.nmp, W.poff, W.cursor, W.pklist);
    for (int a = 1; a < W.ne; ++a) {
        const PslBaEdge &x = W.ed[W.pklist[a - 1]], &y = W.ed[W.pklist[a]];
        if (x.point == y.point && x.kf == y.kf) return PSLFE_E_INVALID;
    }
    return PSLFE_OK;
}

// the same for the LIL edges: the four lists by (keyframe, edge), (LIL, edge), (keyframe, LIL), (LIL, keyframe)
static inline void psl_ba_lil_sort_host(const PslBaLilEdge* led, int nle, const int32_t* src, int by_lil, int nkeys, int32_t* off, int32_t* cursor,
                                        int32_t* dst) {
    for (int k = 0; k <= nkeys; ++k) off[k] = 0;
    for (int e = 0; e < nle; ++e) ++off[(by_lil ? led[e].lil : led[e].kf) + 1];
    for (int k = 0; k < nkeys; ++k) off[k + 1] += off[k];
    for (int k = 0; k < nkeys; ++k) cursor[k] = off[k];
    for (int a = 0; a < nle; ++a) {
        const int e = src ? src[a] : a;
        dst[cursor[by_lil ? led[e].lil : led[e].kf]++] = e;
    }
}
static inline int psl_ba_lil_lists_host(const PslBaWs& W) {
    psl_ba_lil_sort_host(W.led, W.nle, nullptr, 0, W.nkf, W.lkoff, W.cursor, W.lklist);
    psl_ba_lil_sort_host(W.led, W.nle, nullptr, 1, W.nlil, W.lloff, W.cursor, W.lllist);
    psl_ba_lil_sort_host(W.led, W.nle, W.lllist, 0, W.nkf, W.lkoff, W.cursor, W.lkllist);
    psl_ba_lil_sort_host(W.led, W.nle, W.lklist, 1, W.nlil, W.lloff, W.cursor, W.llklist);
    for (int a = 1; a < W.nle; ++a) {
        const PslBaLilEdge &x = W.led[W.llklist[a - 1]], &y = W.led[W.llklist[a]];
        if (x.lil == y.lil && x.kf == y.kf) return PSLFE_E_INVALID;
    }
    return PSLFE_OK;
}
#endif

#endif
