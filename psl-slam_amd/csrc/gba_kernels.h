// Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:37-237): one problem over the whole map.  Product code.
// Plain C++ text, as ba_kernels.h: pslfe_gba.hip includes it for the device and tools/dropin/gba_main.cpp for one core.
//
// Who owns what.  The arithmetic is ba_kernels.h's, called and not copied: psl_ba_edge (its GBA = true instantiation reads the
// deltas of :85-86), psl_ba_build_pose<false>, psl_ba_build_point, psl_ba_point_inverse, psl_ba_schur_term, psl_ba_bschur<false>,
// psl_ba_point_step, psl_ba_chi_partial<false>, psl_po_exp / psl_po_mul.  The loop is psl_lm_levenberg of lm_kernels.h.  This file
// owns the driver psl_gba_optimize and its `Problem`, PslGbaProblem: one optimize(iterations) call, no levels, no erase pass, the
// round trip of every keyframe, vbNotIncludedMP.  Its steps are closures that hold the workspace BY VALUE (PslGbaWs is a struct of
// pointers), so an executor may carry a step across a kernel launch: PslLmGrid of lm_grid.h runs each step as a launch over the
// whole device, PslLmSerial of lm_kernels.h runs the same driver on one core.
//
// Steps with a form of their own at this size; each gives the bits of the one-core text it replaces:
//   the Schur complement   psl_gba_schur_pair: one index per block pair (i1 <= i2) forms the block's entries in ONE merge of the two
//                          (keyframe, point) lists; every entry still subtracts its landmarks in ascending point row
//                          (psl_ba_schur_entry merges once per entry).  A pair whose point ranges do not meet is not merged at all
//   computeLambdaInit      psl_gba_lambda_segment / _fold: 256 segments in index order, folded in order.  `m = a < m ? m : a` is a
//                          maximum but for a NaN, which replaces m and is replaced by the next value; a segment's summary (value,
//                          saw a NaN, not empty) keeps exactly that
//   the pose-index prefix  256 segment counts, their prefix, the assignment
//   computeScale           the products x (lambda x + b) in parallel into a dense buffer (an inactive point holds +0.0, which leaves
//                          a running sum that started at +0.0 unchanged bit for bit), then ONE chain of additions: psl_gba_chain
//   the LDLt, the two substitutions and the chain   psl_gba_factor, psl_gba_forward, psl_gba_backward, psl_gba_chain are the
//                          one-core texts here; an executor may overload them (lm_grid.h does: column panels through LDS, rows
//                          behind a solved diagonal panel, products in parallel and one chain of additions fed from LDS).  Every
//                          L[i][j] is (A[i][j] - sum_k L[i][k] (L[j][k] D[k])) / d_j with k ascending and the product L[j][k] D[k]
//                          rounded first; y[i] = bs[i] - sum_{k<i} L[i][k] y[k], k ascending; x[i] = y[i] / D[i] - sum_{k>i}
//                          L[k][i] x[k], k ascending from i + 1
#ifndef PSL_GBA_KERNELS_H
#define PSL_GBA_KERNELS_H

#include "ba_kernels.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

// a step that may cross a kernel launch
#if defined(__HIPCC__) || defined(__HIP__)
#define PSL_GBA_STEP __host__ __device__
#else
#define PSL_GBA_STEP
#endif

#define PSL_GBA_SEGS PSL_LM_LANES   // segments of the ordered folds

// The workspace: the local BA's views and what the whole-device forms add.  Passed to every step by value.
struct PslGbaWs {
    PslBaWs B;
    double* prod;     // [6 nkf + 3 nmp] the products of computeScale
    double* seg;      // [3 * 256] the segment summaries of computeLambdaInit
    int32_t* segc;    // [256 + 1] the segment counts of the pose-index prefix
    int32_t* kpp;     // [ne] the point row of kplist[a]: the merge of psl_gba_schur_pair reads it without the edge row
};

PSL_BA_HD size_t psl_gba_carve(char* base, int ckf, int cmp, int ced, PslGbaWs* G) {
    size_t off = psl_ba_carve(base, ckf, cmp, ced, &G->B);
    G->prod = reinterpret_cast<double*>(base + psl_ba_take(&off, (6 * (size_t)ckf + 3 * (size_t)cmp) * sizeof(double)));
    G->seg = reinterpret_cast<double*>(base + psl_ba_take(&off, 3 * PSL_GBA_SEGS * sizeof(double)));
    G->segc = reinterpret_cast<int32_t*>(base + psl_ba_take(&off, (PSL_GBA_SEGS + 1) * sizeof(int32_t)));
    G->kpp = reinterpret_cast<int32_t*>(base + psl_ba_take(&off, (size_t)ced * sizeof(int32_t)));
    return off;
}

// segment s of n indices in 256 contiguous segments: [*t0, *t1)
PSL_BA_HD void psl_gba_segment(int n, int s, int* t0, int* t1) {
    const int len = (n + PSL_GBA_SEGS - 1) / PSL_GBA_SEGS;
    const long long a = (long long)s * len, b = a + len;
    *t0 = (int)(a < n ? a : n);
    *t1 = (int)(b < n ? b : n);
}

// ---- the Schur complement, a block pair at a time ----------------------------------------------------------------------------------
// t < F F names (i1, i2); pairs below the diagonal are not formed.  The entries (r, c) of the block (c >= r on the diagonal block)
// are those of psl_ba_schur_entry: Hpp (+ lambda) or 0.0, then minus psl_ba_schur_term of every common landmark in ascending point
// row.
PSL_BA_HD void psl_gba_schur_pair(const PslGbaWs& G, int F, int t, double lambda) {
    const PslBaWs& W = G.B;
    const int i1 = t / F, i2 = t % F;
    if (i2 < i1) return;
    const int N = 6 * F, diag = i1 == i2;
    double s[36];
    PSL_LM_UNROLL
    for (int r = 0; r < 6; ++r)
        PSL_LM_UNROLL
        for (int c = 0; c < 6; ++c) {
            double v = 0.0;
            if (diag && c >= r) {
                v = W.Hpp[21 * (size_t)i1 + psl_ba_tri(6, r, c)];
                if (r == c) v = v + lambda;
            }
            s[6 * r + c] = v;
        }
    const int k1 = W.kfof[i1], k2 = W.kfof[i2];
    int a = W.koff[k1], b = W.koff[k2];
    const int a1 = W.koff[k1 + 1], b1 = W.koff[k2 + 1];
    // both lists ascend in point row: ranges that do not meet have no common landmark
    if (a < a1 && b < b1 && !(G.kpp[a1 - 1] < G.kpp[b] || G.kpp[b1 - 1] < G.kpp[a])) {
        while (a < a1 && b < b1) {
            const int pa = G.kpp[a], pb = G.kpp[b];
            if (pa < pb) { ++a; continue; }
            if (pb < pa) { ++b; continue; }
            const int ea = W.kplist[a], eb = W.kplist[b];
            if (!W.level[ea] && !W.level[eb]) {
                PSL_LM_UNROLL
                for (int r = 0; r < 6; ++r)
                    PSL_LM_UNROLL
                    for (int c = 0; c < 6; ++c)
                        if (!diag || c >= r) s[6 * r + c] = s[6 * r + c] - psl_ba_schur_term(W, ea, eb, r, c);
            }
            ++a; ++b;
        }
    }
    PSL_LM_UNROLL
    for (int r = 0; r < 6; ++r)
        PSL_LM_UNROLL
        for (int c = 0; c < 6; ++c)
            if (!diag || c >= r) W.S[(size_t)(6 * i1 + r) * N + (6 * i2 + c)] = s[6 * r + c];
}

// ---- computeLambdaInit in segments -------------------------------------------------------------------------------------------------
// entry t < 6 F + 3 nmp of psl_ba_lambda_init's sequence: 1 and its magnitude, or 0 for a point that is not active
PSL_BA_HD int psl_gba_diag_entry(const PslBaWs& W, int F, int t, double* a) {
    if (t < 6 * F) {
        *a = __builtin_fabs(W.Hpp[21 * (size_t)(t / 6) + psl_ba_tri(6, t % 6, t % 6)]);
        return 1;
    }
    const int p = (t - 6 * F) / 3, j = (t - 6 * F) % 3;
    if (!W.pact[p]) return 0;
    *a = __builtin_fabs(W.Hll[6 * (size_t)p + psl_ba_tri(3, j, j)]);
    return 1;
}
PSL_BA_HD void psl_gba_lambda_segment(const PslGbaWs& G, int F, int s) {
    int t0, t1;
    psl_gba_segment(6 * F + 3 * G.B.nmp, s, &t0, &t1);
    double m = 0.0;
    int nan = 0, any = 0;
    for (int t = t0; t < t1; ++t) {
        double a;
        if (!psl_gba_diag_entry(G.B, F, t, &a)) continue;
        any = 1;
        if (a != a) nan = 1;
        m = a < m ? m : a;
    }
    G.seg[3 * s] = m; G.seg[3 * s + 1] = (double)nan; G.seg[3 * s + 2] = (double)any;
}
PSL_BA_HD double psl_gba_lambda_fold(const PslGbaWs& G) {
    double m = 0.0;
    for (int s = 0; s < PSL_GBA_SEGS; ++s) {
        if (G.seg[3 * s + 2] == 0.0) continue;
        const double r = G.seg[3 * s];
        if (G.seg[3 * s + 1] != 0.0) m = r;   // the values behind the segment's last NaN, or that NaN: what came before is gone
        else m = r < m ? m : r;               // a NaN m is replaced by the segment's first value: r, the maximum of magnitudes
    }
    return 1e-5 * m;
}

// ---- the dense solve: the one-core texts (lm_grid.h overloads them for the whole device) ------------------------------------------
// An executor that brings forms of its own for the four steps below declares `static constexpr bool tiled_solve = true` and
// overloads all four; should one of its overloads stop matching, the generic text must not run in its place unnoticed (it gives
// the same bits, so no parity test would see it): the generic texts refuse such an executor at compile time.
template <class Exec, class = void>
struct PslGbaTiled { static constexpr bool value = false; };
template <class Exec>
struct PslGbaTiled<Exec, decltype((void)Exec::tiled_solve)> { static constexpr bool value = Exec::tiled_solve; };
#define PSL_GBA_GENERIC_ONLY(Exec) static_assert(!PslGbaTiled<Exec>::value, "this executor declares tiled_solve: its own overload of this step must be the one that is called")
// The LDLt of S in place, psl_ba_solve's: a column at a time, c[k] = L[j][k] D[k] rounded first.  A pivot that is not a finite
// positive number clears W.flag[0].
template <class Exec>
PSL_BA_HD void psl_gba_factor(Exec& X, const PslGbaWs& G, int N) {
    PSL_GBA_GENERIC_ONLY(Exec);
    const PslBaWs W = G.B;
    for (int j = 0; j < N; ++j) {
        X.par(j, [W, N, j] PSL_GBA_STEP(int k) { W.cc[k] = W.S[(size_t)j * N + k] * W.Dd[k]; });
        X.par(N - j, [W, N, j] PSL_GBA_STEP(int t) {
            const int i = j + t;
            double d = W.S[(size_t)j * N + j];
            for (int k = 0; k < j; ++k) d = d - W.S[(size_t)j * N + k] * W.cc[k];
            if (i == j) {
                if (!(d > 0.0) || !(d <= PSL_LM_DBL_MAX)) W.flag[0] = 0;
                W.Dd[j] = d;
                return;
            }
            double s = W.S[(size_t)j * N + i];
            for (int k = 0; k < j; ++k) s = s - W.S[(size_t)i * N + k] * W.cc[k];
            W.S[(size_t)i * N + j] = PSL_LM_DIV(s, d);
        });
    }
}
// L y = bs: y in W.cc
template <class Exec>
PSL_BA_HD void psl_gba_forward(Exec& X, const PslGbaWs& G, int N) {
    PSL_GBA_GENERIC_ONLY(Exec);
    const PslBaWs W = G.B;
    X.one([W, N] PSL_GBA_STEP() {
        for (int i = 0; i < N; ++i) {
            double s = W.bs[i];
            for (int k = 0; k < i; ++k) s = s - W.S[(size_t)i * N + k] * W.cc[k];
            W.cc[i] = s;
        }
    });
}
// x = D^-1 y - L^T x: x in W.xp
template <class Exec>
PSL_BA_HD void psl_gba_backward(Exec& X, const PslGbaWs& G, int N) {
    PSL_GBA_GENERIC_ONLY(Exec);
    const PslBaWs W = G.B;
    X.one([W, N] PSL_GBA_STEP() {
        for (int i = N - 1; i >= 0; --i) {
            double s = PSL_LM_DIV(W.cc[i], W.Dd[i]);
            for (int k = i + 1; k < N; ++k) s = s - W.S[(size_t)k * N + i] * W.xp[k];
            W.xp[i] = s;
        }
    });
}
// *out = ((0.0 + buf[0]) + buf[1]) + ... + buf[n - 1]
template <class Exec>
PSL_BA_HD void psl_gba_chain(Exec& X, const PslGbaWs&, const double* buf, int n, double* out) {
    PSL_GBA_GENERIC_ONLY(Exec);
    X.one([buf, n, out] PSL_GBA_STEP() {
        double s = 0.0;
        for (int j = 0; j < n; ++j) s = s + buf[j];
        *out = s;
    });
}

// BlockSolver::solve at `lambda`, as psl_ba_solve<false>: 1 and xp, xl, or 0, "the solve failed"
template <class Exec>
PSL_BA_HD int psl_gba_solve(Exec& X, const PslGbaWs& G, int F, double lambda) {
    const PslBaWs W = G.B;
    const int N = 6 * F;
    int32_t* ok = W.flag;
    X.one([ok] PSL_GBA_STEP() { *ok = 1; });
    X.par(W.nmp, [W, lambda, ok] PSL_GBA_STEP(int p) { psl_ba_point_inverse(W, p, lambda, ok); });
    if (!X.get(ok)) return 0;
    X.par(F * F, [G, F, lambda] PSL_GBA_STEP(int t) { psl_gba_schur_pair(G, F, t, lambda); });
    X.par(N, [W] PSL_GBA_STEP(int t) { psl_ba_bschur<false>(W, t); });
    psl_gba_factor(X, G, N);
    if (!X.get(ok)) return 0;
    psl_gba_forward(X, G, N);
    psl_gba_backward(X, G, N);
    X.par(F, [W, ok] PSL_GBA_STEP(int i) { if (!psl_lm_step_ok(W.xp + 6 * (size_t)i)) *ok = 0; });
    if (!X.get(ok)) return 0;
    X.par(W.nmp, [W] PSL_GBA_STEP(int p) { psl_ba_point_step(W, p); });
    return 1;
}

// The `Problem` of psl_lm_levenberg for Optimizer::BundleAdjustment: PslBaProblem<false>'s steps with the workspace by value, the
// deltas of :85-86 and the forms above.
struct PslGbaProblem {
    PslGbaWs G;
    int F, robust;
    template <class Exec> PSL_LM_MEMBER double linearize(Exec& X, double* chi_first) {
        const PslBaWs W = G.B;
        const int robust_ = robust;
        X.par(W.ne, [W, robust_] PSL_GBA_STEP(int e) { psl_ba_edge<true>(W, e, W.T, W.X, robust_, 1); });
        const double chi = X.sum256([W] PSL_GBA_STEP(int p) { return psl_ba_chi_partial<false>(W, p); });
        if (chi_first) *chi_first = chi;
        X.par(27 * F, [W] PSL_GBA_STEP(int t) { psl_ba_build_pose<false>(W, t); });
        X.par(9 * W.nmp, [W] PSL_GBA_STEP(int t) { psl_ba_build_point(W, t); });
        return chi;
    }
    template <class Exec> PSL_LM_MEMBER double lambda_init(Exec& X) {
        const PslGbaWs G_ = G;
        const int F_ = F;
        X.par(PSL_GBA_SEGS, [G_, F_] PSL_GBA_STEP(int s) { psl_gba_lambda_segment(G_, F_, s); });
        X.one([G_] PSL_GBA_STEP() { G_.B.scal[0] = psl_gba_lambda_fold(G_); });
        return X.get(G_.B.scal);
    }
    template <class Exec> PSL_LM_MEMBER int solve(Exec& X, double lambda) { return psl_gba_solve(X, G, F, lambda); }
    template <class Exec> PSL_LM_MEMBER double candidate(Exec& X) {
        const PslBaWs W = G.B;
        const int robust_ = robust;
        X.par(W.nkf + W.nmp, [W] PSL_GBA_STEP(int v) {   // oplusImpl of every active vertex
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
        X.par(W.ne, [W, robust_] PSL_GBA_STEP(int e) { psl_ba_edge<true>(W, e, W.Tn, W.Xn, robust_, 0); });
        return X.sum256([W] PSL_GBA_STEP(int p) { return psl_ba_chi_partial<false>(W, p); });
    }
    template <class Exec> PSL_LM_MEMBER double scale(Exec& X, double lambda) {
        const PslGbaWs G_ = G;
        const int n6 = 6 * F;
        X.par(n6 + 3 * G_.B.nmp, [G_, n6, lambda] PSL_GBA_STEP(int j) {   // the terms of psl_ba_scale, each rounded once
            const PslBaWs& W = G_.B;
            if (j < n6) { G_.prod[j] = W.xp[j] * (lambda * W.xp[j] + W.bp[j]); return; }
            const int q = j - n6;
            if (!W.pact[q / 3]) { G_.prod[j] = 0.0; return; }
            const double x = W.xl[q];
            G_.prod[j] = x * (lambda * x + W.bl[q]);
        });
        psl_gba_chain(X, G_, G_.prod, n6 + 3 * G_.B.nmp, G_.B.scal + 1);
        return X.get(G_.B.scal + 1);
    }
    template <class Exec> PSL_LM_MEMBER void accept(Exec& X) {   // discardTop: the candidate becomes the estimate
        const PslBaWs W = G.B;
        X.par(W.nkf + W.nmp, [W] PSL_GBA_STEP(int v) {
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

// What a call reports besides the rows (PslGbaInfo of include/pslfe.h without its status)
struct PslGbaResult {
    int iterations, free_keyframes, included_points;
    double chi2_start, chi2_end, lambda;
};

// Optimizer::BundleAdjustment on a checked problem whose four lists are built: the estimates from the rows (toSE3Quat, toVector3d),
// initializeOptimization() (a vertex without an edge is not in the system; a fixed keyframe gets no block), one
// optimize(iterations) with Huber on every edge (robust) or on none, then the rows out: EVERY keyframe gets toCvMat of its SE3Quat,
// the fixed ones and those without an edge too (:193-210); not_included[p] = vbNotIncludedMP (:175-183); an included point gets
// (float) of its estimate, the others keep their row.  No edge, or no free keyframe in the system: no iteration.
// kf_out / mp_out may be the input rows.  The decisions are taken where the executor's get / sum256 return: on the caller's thread.
template <class Exec>
PSL_BA_HD PslGbaResult psl_gba_optimize(Exec& X, const PslGbaWs& G, int iterations, int robust, PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out,
                                        uint8_t* not_included) {
    const PslBaWs W = G.B;
    X.par(W.nkf + W.nmp + W.ne, [W, G] PSL_GBA_STEP(int v) {
        if (v < W.nkf) {
            psl_po_from_pose(W.kf[v].Tcw.R, W.kf[v].Tcw.t, &W.T[v]);
            W.Tn[v] = W.T[v];
            W.pidx[v] = W.koff[v + 1] > W.koff[v] && !W.kf[v].fixed ? 0 : -1;
        } else if (v < W.nkf + W.nmp) {
            const int p = v - W.nkf;
            const double x[3] = {(double)W.mp[p].x, (double)W.mp[p].y, (double)W.mp[p].z};
            for (int j = 0; j < 3; ++j) { W.X[3 * (size_t)p + j] = x[j]; W.Xn[3 * (size_t)p + j] = x[j]; }
            W.pact[p] = (uint8_t)(W.poff[p + 1] > W.poff[p]);
        } else {
            const int e = v - W.nkf - W.nmp;
            W.level[e] = 0;
            W.err[3 * (size_t)e] = 0.0; W.err[3 * (size_t)e + 1] = 0.0; W.err[3 * (size_t)e + 2] = 0.0;
            W.rho0[e] = 0.0;
            G.kpp[e] = W.ed[W.kplist[e]].point;
        }
    });
    // the pose index: a prefix count in row order, in segments
    X.par(PSL_GBA_SEGS, [G] PSL_GBA_STEP(int s) {
        int t0, t1, n = 0;
        psl_gba_segment(G.B.nkf, s, &t0, &t1);
        for (int k = t0; k < t1; ++k) n += G.B.pidx[k] >= 0;
        G.segc[s + 1] = n;
    });
    X.one([G] PSL_GBA_STEP() {
        G.segc[0] = 0;
        for (int s = 0; s < PSL_GBA_SEGS; ++s) G.segc[s + 1] += G.segc[s];
        G.B.flag[1] = G.segc[PSL_GBA_SEGS];
    });
    X.par(PSL_GBA_SEGS, [G] PSL_GBA_STEP(int s) {
        int t0, t1, n = G.segc[s];
        psl_gba_segment(G.B.nkf, s, &t0, &t1);
        for (int k = t0; k < t1; ++k)
            if (G.B.pidx[k] >= 0) { G.B.pidx[k] = n; G.B.kfof[n] = k; ++n; }
    });
    PslGbaResult R = {0, X.get(W.flag + 1), 0, 0.0, 0.0, 0.0};
    if (R.free_keyframes > 0 && W.ne > 0) {
        PslGbaProblem P = {G, R.free_keyframes, robust};
        R.iterations = psl_lm_levenberg(X, P, iterations, &R.chi2_start, &R.chi2_end, &R.lambda);
    }
    R.included_points = (int)X.sum256([W] PSL_GBA_STEP(int p) {   // a count: exact in any order
        double s = 0.0;
        for (int q = p; q < W.nmp; q += PSL_LM_LANES) s = s + (W.pact[q] ? 1.0 : 0.0);
        return s;
    });
    X.par(W.nkf + W.nmp, [W, kf_out, mp_out, not_included] PSL_GBA_STEP(int v) {
        if (v < W.nkf) {
            PslBaKeyFrame o = W.kf[v];
            psl_po_to_pose(&W.T[v], o.Tcw.R, o.Tcw.t);   // SetPose / mTcwGBA of every keyframe
            kf_out[v] = o;
        } else {
            const int p = v - W.nkf;
            PslMapPointGeom o = W.mp[p];
            if (W.pact[p]) { o.x = (float)W.X[3 * (size_t)p]; o.y = (float)W.X[3 * (size_t)p + 1]; o.z = (float)W.X[3 * (size_t)p + 2]; }
            mp_out[p] = o;
            not_included[p] = (uint8_t)!W.pact[p];
        }
    });
    return R;
}

#endif
