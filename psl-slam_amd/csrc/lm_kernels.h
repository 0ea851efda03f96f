// g2o's Levenberg loop: the driver psl_lm_levenberg (one optimize() call: the iterations, the trials of an iteration and every
// decision g2o makes between two sums) over an executor and a `Problem`, and, as functions of one thread, what one vertex needs: the
// LDLt solve in N unknowns, lambda, rho, the Huber kernel and psl_lm_optimize, the driver on one vertex.  Product code, shared by the
// pose optimisation (pose_kernels.h, N = 6), OptimizeSim3 (sim3_kernels.h, N = 7), the local bundle adjustment (ba_kernels.h) and
// the essential graph (essential_kernels.h).  Plain C++ text: the kernels include it for the device and the host loops of
// tools/dropin for one core, so all run the same single IEEE operations (build with -ffp-contract=off).  The driver knows neither
// the vertices nor how a sum is formed or a system solved: it asks its `Problem` argument.  k_ba_local, k_eg_optimize and all five
// host loops instantiate it; k_pose_optimize and k_sim3_optimize call the primitives here but hold the driver's loop written out
// (instantiating it there cost 0.6 to 1.9 % per launch: profiles/pose_driver_ab.json, the headers of pslfe_pose.hip and
// pslfe_sim3.hip).  So the loop has three texts that are changed together: the driver psl_lm_levenberg, and the two loops written
// out in k_pose_optimize and k_sim3_optimize.  Restated from the reference's g2o:
//   one iteration, the loop   Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189, sparse_optimizer.cpp:354-419
//   Huber                     Thirdparty/g2o/g2o/core/robust_kernel_impl.cpp:78-92
// tests/lm_cases.py is the same loop in numpy.  DESIGN.md §5.0k, §5.0l.
#ifndef PSL_LM_KERNELS_H
#define PSL_LM_KERNELS_H

#if defined(__HIPCC__) || defined(__HIP__)
#include <hip/hip_runtime.h>
#define PSL_LM_HD __host__ __device__ static inline
#define PSL_LM_MEMBER __host__ __device__
#else
#define PSL_LM_HD static inline
#define PSL_LM_MEMBER
#endif
#include <stdint.h>

#ifdef __clang__
#pragma clang fp contract(off)
#endif

// division and square root: the correctly rounded device intrinsics, as csrc/proj_kernels.h takes them
#if defined(__HIP_DEVICE_COMPILE__)
#define PSL_LM_DIV(a, b) __ddiv_rn((a), (b))
#define PSL_LM_SQRT(a) __dsqrt_rn(a)
#else
#define PSL_LM_DIV(a, b) ((a) / (b))
#define PSL_LM_SQRT(a) __builtin_sqrt(a)
#endif

// full unrolling keeps the small arrays of the solve in registers on the device (indices become constants); the solve in seven
// unknowns needs it (profiles/sim3_codegen.txt), the one in six compiles to the same code with and without it
#ifdef __clang__
#define PSL_LM_UNROLL _Pragma("unroll")
#else
#define PSL_LM_UNROLL
#endif

#define PSL_LM_LANES 256   // partial sums of the ordered reduction (the headers of pslfe_pose.hip and pslfe_sim3.hip)
#define PSL_LM_GROUP 64    // partial sums of one butterfly
#define PSL_LM_DBL_MAX 1.79769313486231570815e+308

// Steps 2 and 3 of the order of the sums on the 256 partial sums of one value, on one core: the butterfly inside each group of 64,
// then ((G0 + G1) + G2) + G3.  (On the device: psl_lm_reduce of lm_device.h.)
PSL_LM_HD double psl_lm_reduce_lanes(double* part) {
    double G[PSL_LM_LANES / PSL_LM_GROUP];
    for (int g = 0; g < PSL_LM_LANES / PSL_LM_GROUP; ++g) {
        double* p = part + g * PSL_LM_GROUP;
        for (int s = PSL_LM_GROUP / 2; s >= 1; s >>= 1)
            for (int l = 0; l < s; ++l) p[l] = p[l] + p[l + s];
        G[g] = p[0];
    }
    return ((G[0] + G[1]) + G[2]) + G[3];
}

// RobustKernelHuber::robustify (robust_kernel_impl.cpp:78-92): rho(chi2) and rho'(chi2).  delta: what the caller's setDelta got.
PSL_LM_HD void psl_lm_huber(double chi2, double delta, double* rho0, double* rho1) {
    const double dsqr = delta * delta;
    if (chi2 <= dsqr) { *rho0 = chi2; *rho1 = 1.0; }
    else {
        const double sq = PSL_LM_SQRT(chi2);
        *rho0 = (2.0 * sq) * delta - dsqr;
        *rho1 = PSL_LM_DIV(delta, sq);
    }
}

// (H + lambda I) x = b by LDLt without pivoting; H: the N (N + 1) / 2 upper-triangle values row by row.  Returns 0 - "the solve
// failed" - when a pivot is not a finite positive number (the matrix is then not positive definite to working precision); x is not
// written then.
template <int N>
PSL_LM_HD int psl_lm_solve(const double* H, double lambda, const double* b, double* x) {
    double A[N][N], L[N][N], D[N], y[N];
    int h = 0;
    PSL_LM_UNROLL
    for (int j = 0; j < N; ++j)
        PSL_LM_UNROLL
        for (int k = j; k < N; ++k, ++h) { A[j][k] = H[h]; A[k][j] = H[h]; }
    PSL_LM_UNROLL
    for (int j = 0; j < N; ++j) A[j][j] = A[j][j] + lambda;
    int ok = 1;
    PSL_LM_UNROLL
    for (int j = 0; j < N; ++j) {
        double d = A[j][j];
        PSL_LM_UNROLL
        for (int k = 0; k < j; ++k) d = d - L[j][k] * (L[j][k] * D[k]);
        if (!(d > 0.0) || !(d <= PSL_LM_DBL_MAX)) ok = 0;
        D[j] = d;
        PSL_LM_UNROLL
        for (int i = j + 1; i < N; ++i) {
            double s = A[i][j];
            PSL_LM_UNROLL
            for (int k = 0; k < j; ++k) s = s - L[i][k] * (L[j][k] * D[k]);
            L[i][j] = PSL_LM_DIV(s, d);
        }
    }
    if (!ok) return 0;
    PSL_LM_UNROLL
    for (int i = 0; i < N; ++i) {
        double s = b[i];
        PSL_LM_UNROLL
        for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    PSL_LM_UNROLL
    for (int i = N - 1; i >= 0; --i) {
        double s = PSL_LM_DIV(y[i], D[i]);
        PSL_LM_UNROLL
        for (int k = i + 1; k < N; ++k) s = s - L[k][i] * x[k];
        x[i] = s;
    }
    return 1;
}

// The rotation angle of a step, |omega| = |x[0..2]| for both vertex types, must lie inside the range of psl_glibc_sin /
// psl_glibc_cos (their table index is not clamped).  A step outside it - or a NaN one - only comes from non-physical data and
// counts as "the solve failed".
#define PSL_LM_THETA_MAX 105414350.0
PSL_LM_HD int psl_lm_step_ok(const double* x) {
    const double theta = PSL_LM_SQRT((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]);
    return theta < PSL_LM_THETA_MAX;
}

// computeLambdaInit (optimization_algorithm_levenberg.cpp:166-180): tau * max |H_jj|
template <int N>
PSL_LM_HD double psl_lm_lambda_init(const double* H) {
    double m = 0.0;
    int h = 0;
    for (int j = 0; j < N; h += N - j, ++j) {
        const double a = __builtin_fabs(H[h]);
        m = a < m ? m : a;   // std::max(fabs(h), m)
    }
    return 1e-5 * m;
}

// rho of one trial (:129-132): (chi - chi_new) / (sum x_j (lambda x_j + b_j) + 1e-3)
template <int N>
PSL_LM_HD double psl_lm_rho(double chi, double chi_new, const double* x, const double* b, double lambda) {
    double scale = 0.0;
    for (int j = 0; j < N; ++j) scale = scale + x[j] * (lambda * x[j] + b[j]);
    scale = scale + 1e-3;
    return PSL_LM_DIV(chi - chi_new, scale);
}

// the lambda factor of an accepted step (:135-139): 1 - (2 rho - 1)^3 clamped to [1/3, 2/3]; the cube is two products
PSL_LM_HD double psl_lm_good_scale(double rho) {
    const double t = 2.0 * rho - 1.0;
    double alpha = 1.0 - (t * t) * t;
    alpha = (2.0 / 3.0) < alpha ? (2.0 / 3.0) : alpha;    // std::min(alpha, upper)
    return (1.0 / 3.0) < alpha ? alpha : (1.0 / 3.0);     // std::max(lower, alpha)
}

// One optimize(iterations) call of g2o: up to `iterations` Levenberg iterations of up to ten trials, with every decision g2o makes
// between two sums and nothing else.  What is optimised, and on what it runs, are the two arguments.
//
// The executor `Exec` runs the steps of a Problem; this is its whole contract:
//   par(n, f)      f(0) .. f(n - 1), independent of each other; all of them are done before the next step starts
//   one(f)         f() once, done before the next step starts
//   sum256(f)      the ordered sum of the 256 partial sums f(0) .. f(255): a butterfly in each group of 64, then ((G0 + G1) + G2) + G3
//   get(p)         the value at p, the same for every caller, read before anybody writes there again
// PslLmSerial below runs them on one core (sum256 through psl_lm_reduce_lanes); PslLmWorkgroup of lm_device.h spreads par over the
// 256 threads of a workgroup with a barrier after it (sum256 through psl_lm_reduce).  A Problem whose steps are functions of
// (workspace, index) that write only what the index owns does not depend on how the indices are spread, so the two executors give
// the same bits by construction.
//
// The `Problem` holds the estimate and a candidate for it and supplies what differs between the optimisers, each a template over Exec:
//   linearize(X, chi_first)   the errors and Jacobians at the estimate, the ordered sum of the robust chi2 of the active edges, then H
//                             and b.  Returns that chi2 and, where chi_first is not NULL, also writes it there
//   lambda_init(X)            the lambda of iteration 0 (computeLambdaInit, :166-180)
//   solve(X, lambda)          (H + lambda I) x = b: 1 and the step x, or 0, "the solve failed"
//   candidate(X)              oplus(estimate, x) on every vertex and the errors there.  Returns the robust chi2 at the candidate
//   scale(X, lambda)          computeScale: sum x_j (lambda x_j + b_j) in index order, of the x that candidate left
//   accept(X)                 the candidate becomes the estimate
// lambda, ni and _nBad are initialised by each call.  A failed solve makes the trial's chi2 DBL_MAX with a zero step in rho (:120):
// no candidate is formed, the trial is rejected and lambda grows.  chi_first: the chi2 of iteration 0; chi_last: the current chi2
// when the call returns; lambda_out: the lambda then.  Returns the iterations run.
template <class Exec, class Problem>
PSL_LM_HD int psl_lm_levenberg(Exec& X, Problem& P, int iterations, double* chi_first, double* chi_last, double* lambda_out) {
    int its = 0;
    double lambda = 0.0, ni = 2.0;
    int nbad = 0;   // _nBad: iterations in a row that gained less than 1e-3 of their chi2
    for (int it = 0; it < iterations; ++it) {
        double chi = P.linearize(X, it == 0 ? chi_first : nullptr);
        const double ini_chi = chi;
        if (it == 0) { lambda = P.lambda_init(X); ni = 2.0; nbad = 0; }
        double rho = 0.0;
        int qmax = 0;
        do {
            const int ok = P.solve(X, lambda);
            double temp_chi = PSL_LM_DBL_MAX;   // a failed solve (:120)
            double scale = 0.0;                 // ... has a zero step in rho
            if (ok) {
                temp_chi = P.candidate(X);
                scale = P.scale(X, lambda);
            }
            scale = scale + 1e-3;
            rho = PSL_LM_DIV(chi - temp_chi, scale);   // (:129-132)
            if (rho > 0 && __builtin_fabs(temp_chi) <= PSL_LM_DBL_MAX) {
                lambda = lambda * psl_lm_good_scale(rho);
                ni = 2.0;
                chi = temp_chi;
                if (ok) P.accept(X);   // a failed solve has no candidate: the estimate stays (chi = inf reaches this)
            } else {
                lambda = lambda * ni;
                ni = ni * 2.0;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);
        ++its;
        *chi_last = chi;
        if (qmax == 10 || rho == 0) break;                               // Terminate
        if ((ini_chi - chi) * 1e3 < ini_chi) ++nbad; else nbad = 0;      // the _nBad rule
        if (nbad >= 3) break;
    }
    *lambda_out = lambda;
    return its;
}

// psl_lm_levenberg on one vertex of N unknowns, on one core.  Problem holds the estimate and a candidate for it and supplies what
// depends on the vertex type and on the sums:
//   sums(acc)       the N (N + 1) / 2 values of H (upper triangle, row by row), the N of b (before the sign) and the robust chi2
//                   of the active edges at the estimate, summed in the Problem's own, fixed order
//   candidate(x)    forms the candidate, oplus(estimate, x).  It may edit x: what it leaves there enters rho, as g2o's computeScale
//                   reads the solver's own vector after oplusImpl has written into it
//   chi()           the robust chi2 of the active edges at the candidate
//   accept()        the candidate becomes the estimate
// A step whose angle psl_lm_step_ok refuses counts as a failed solve.  Returns the iterations run.
template <int N, class Problem>
PSL_LM_HD int psl_lm_optimize(Problem& P, int iterations);

#if !defined(__HIP_DEVICE_COMPILE__)   // the host loops only; the device pass sees the declaration above, which psl_po_rounds and psl_s3_rounds name
// the executor of one core
struct PslLmSerial {
    double* part;   // [256]; a Problem that never sums may leave it NULL
    template <class Fn> PSL_LM_MEMBER void par(int n, Fn f) { for (int i = 0; i < n; ++i) f(i); }
    template <class Fn> PSL_LM_MEMBER void one(Fn f) { f(); }
    template <class Fn> PSL_LM_MEMBER double sum256(Fn f) {
        for (int p = 0; p < PSL_LM_LANES; ++p) part[p] = f(p);
        return psl_lm_reduce_lanes(part);
    }
    template <class V> PSL_LM_MEMBER V get(const V* p) { return *p; }
};

// A `Vertex` (the contract of psl_lm_optimize) as a Problem of the driver: the system of one vertex of N unknowns in registers
template <int N, class Vertex>
struct PslLmOneVertex {
    static constexpr int NH = N * (N + 1) / 2;
    Vertex& P;
    double acc[NH + N + 1], b[N], x[N];
    template <class Exec> PSL_LM_MEMBER double linearize(Exec&, double* chi_first) {
        P.sums(acc);
        for (int j = 0; j < N; ++j) b[j] = -acc[NH + j];
        if (chi_first) *chi_first = acc[NH + N];
        return acc[NH + N];
    }
    template <class Exec> PSL_LM_MEMBER double lambda_init(Exec&) { return psl_lm_lambda_init<N>(acc); }
    template <class Exec> PSL_LM_MEMBER int solve(Exec&, double lambda) {
        for (int j = 0; j < N; ++j) x[j] = 0.0;
        int ok = psl_lm_solve<N>(acc, lambda, b, x);
        if (ok && !psl_lm_step_ok(x)) {   // a rotation angle outside the range of the restated sin / cos: as a failed solve
            ok = 0;
            for (int j = 0; j < N; ++j) x[j] = 0.0;
        }
        return ok;
    }
    template <class Exec> PSL_LM_MEMBER double candidate(Exec&) {
        P.candidate(x);
        return P.chi();
    }
    template <class Exec> PSL_LM_MEMBER double scale(Exec&, double lambda) {
        double s = 0.0;
        for (int j = 0; j < N; ++j) s = s + x[j] * (lambda * x[j] + b[j]);
        return s;
    }
    template <class Exec> PSL_LM_MEMBER void accept(Exec&) { P.accept(); }
};

template <int N, class Problem>
PSL_LM_HD int psl_lm_optimize(Problem& P, int iterations) {
    PslLmSerial X = {nullptr};
    PslLmOneVertex<N, Problem> V = {P};
    double chi_first, chi_last, lambda;
    return psl_lm_levenberg(X, V, iterations, &chi_first, &chi_last, &lambda);
}
#endif

#endif
