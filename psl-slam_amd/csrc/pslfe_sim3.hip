// libpslfe: Optimizer::OptimizeSim3 (src/Optimizer.cc:2801-2996, called at src/LoopClosing.cc:326) for K loop candidates in one
// launch, and its set-up loop (:2854-2933).  Product code.
// Reference behaviour restated (in double, in the reference's order of decisions): sim3_kernels.h names every source line.
// Who owns what.  sim3_kernels.h holds the arithmetic of a pair, the numeric Jacobian, the Sim3 update and the two calls
// psl_s3_rounds; lm_kernels.h holds the 7x7 solve, the Huber kernel and the Levenberg driver psl_lm_levenberg, which the pose
// optimisation, the local bundle adjustment and the essential graph share.  The host loop of tools/dropin/sim3_main.cpp
// instantiates psl_s3_rounds and with it psl_lm_optimize<7>, the driver on one vertex.
// k_sim3_optimize calls the same primitives but keeps the two calls and the driver's loop written out (sim3_rounds,
// sim3_optimize and sim3_step below), as k_pose_optimize does: with Sim3DeviceSums as the problem of psl_lm_optimize<7> it had the
// same VGPRs, scratch, spills, LDS and occupancy and the same count of every f64 opcode, but 254 AGPRs for 237, and launched 0.7 to
// 1.8 % slower than this form on an MI355X, outside the parent's own spread in five of six rows (profiles/lm_core_ab.json,
// DESIGN.md §5.0l).  This form compiles to the instructions the kernel had on its own driver.  So the loop has three texts that
// are changed together: the driver psl_lm_levenberg, and the two loops written out in k_pose_optimize and here; a change to
// PslS3Vertex or psl_s3_rounds is likewise a change to those three functions and the reverse.  tests/test_sim3_opt_gpu.py compares
// both with the numpy restatement bit for bit.  The device's own, here: which thread owns which pair, the order of the sums (its
// steps 2 and 3 are psl_lm_reduce of lm_device.h, shared with pslfe_pose.hip), the LDS copy of the rows, the perturbed estimates
// shared through LDS, the error paths, the pair set-up kernel.
//
// Layout.  One workgroup of 256 threads per candidate, resident through both optimize() calls, every iteration and every trial.
// The pair rows (12 floats) of a candidate with at most PSL_S3_LDS_PAIRS pairs are copied to LDS once (48 KB at the capacity; row
// stride 12 words); a larger candidate reads them from HBM, with the same arithmetic.  Thread t owns the PAIRS t, t + 256, ...: both
// edges of a pair share their classification, and the owner alone reads and writes the pair's outlier byte, which says whether
// the pair is still in the graph.
//
// Order of the sums.  H (28 values), b (7) and the robust chi2 of the active pairs are summed in an order fixed by the pair index
// and the pair count alone:
//   1. partial sum p (0 <= p < 256) starts at +0.0 and adds, for the active pairs p, p + 256, ... in ascending order, the terms of
//      the pair's e12 edge and then those of its e21 edge (g2o's edge order);
//   2. inside each group of 64 consecutive partial sums, for s = 32, 16, 8, 4, 2, 1: partial[g*64 + l] += partial[g*64 + l + s] for
//      l < s;
//   3. the four group sums are added as ((G0 + G1) + G2) + G3 (through LDS, stride 36, two alternating buffers, one barrier).
// Nothing depends on the batch or the candidate's position in it.  tests/sim3_opt_cases.py implements the same order in numpy.
//
// Perturbed estimates.  g2o's numeric Jacobian needs the estimate moved by +-1e-9 along each of the 7 axes, and for the e21 edges
// the inverse of each: 14 Sim3 and 14 inverses that depend on the estimate alone.  Threads 0..13 compute one each
// (psl_s3_perturbed) and share them through LDS (1792 bytes) with one barrier per linearisation; all 14 take the same branch of
// the exponential (theta and sigma are 0 or 1e-9), so the wave does not diverge.  Computing them redundantly in every lane gives the
// same bits but keeps 224 doubles live next to the 36 accumulators (profiles/sim3_codegen.txt).
//
// Solve and update are computed redundantly by every lane from the reduced sums, as in pslfe_pose.hip; control flow is uniform.
#include <string.h>

#include "pslfe_internal.h"
#include "match_kernels.h"
#include "proj_kernels.h"
#include "sim3_kernels.h"
#include "lm_device.h"

#define PSL_S3_BS PSL_LM_LANES
#define PSL_S3_LDS_PAIRS 1024   // 48 KB of pair rows

static_assert(sizeof(PslSim3Pair) == PSL_S3_PAIR_FLOATS * sizeof(float), "a pair row is 12 floats");
static_assert(sizeof(PslSim3D) == sizeof(PslS3) && sizeof(PslS3) == 64, "Sim3 as 8 doubles");
static_assert(PSL_S3_BS == 4 * PSL_LM_GROUP, "four waves of 64");

__device__ const double g_s3_sctab[444] = {
#include "psl_sincostab.inc"
};

struct Sim3Args {
    const PslSim3* Sin;
    const PslSim3Pair* pairs;
    const int32_t* npairs;
    int pstride, lds_pairs;
    PslS3Cams K;
    double th2, delta;
    int fix_scale;
    PslSim3D* Sout;
    uint8_t* bad;
    int32_t* nin;
    PslSim3Info* info;
};

// psl_s3_perturbed as a function of its own: inlined, the four branches of the exponential and the restated sin / cos and exp sit
// in the middle of the driver's live values and the register allocator spills around them (profiles/sim3_codegen.txt)
__device__ __noinline__ void psl_s3_perturbed_call(const PslS3* S, int k, int fix_scale, PslS3* Sp, PslS3* Spi) {
    psl_s3_perturbed(S, k, fix_scale, g_s3_sctab, Sp, Spi);
}

// what k_sim3_optimize sums over the pairs of its candidate, on a workgroup
struct Sim3DeviceSums {
    const float* P;       // the pair rows (LDS or HBM)
    uint8_t* out;         // the outlier bytes of the candidate
    int n;
    PslS3Cams K;
    double th2, delta;
    int fix_scale;
    double* s_red;
    PslS3 (*s_pert)[2];
    int flip;
    PslSim3Info* info;

    __device__ __forceinline__ void system(const PslS3& S, const PslS3& Si, double* acc) {
        const int tid = threadIdx.x;
        if (tid < PSL_S3_NPERT) {
            PslS3 a, b;
            psl_s3_perturbed_call(&S, tid, fix_scale, &a, &b);
            s_pert[tid][0] = a;
            s_pert[tid][1] = b;
        }
        __syncthreads();   // the reads below end before the barrier of the reduction; the next linearisation writes after it
#pragma unroll
        for (int k = 0; k < PSL_S3_NTERMS; ++k) acc[k] = 0.0;
        for (int i = tid; i < n; i += PSL_S3_BS) {
            if (out[i]) continue;
            const float* row = P + PSL_S3_PAIR_FLOATS * i;
            psl_s3_edge_terms(row, 0, &S, &Si, s_pert, &K, delta, acc);
            psl_s3_edge_terms(row, 1, &S, &Si, s_pert, &K, delta, acc);
        }
        psl_lm_reduce<PSL_S3_NTERMS, PSL_S3_NTERMS>(acc, s_red, flip);
    }
    __device__ __forceinline__ double chi(const PslS3& S, const PslS3& Si) {
        double cs[1] = {0.0};
        for (int i = threadIdx.x; i < n; i += PSL_S3_BS) {
            if (out[i]) continue;
            const float* row = P + PSL_S3_PAIR_FLOATS * i;
            double e[2], w;
            cs[0] = cs[0] + psl_s3_edge_rho(row, 0, &S, &Si, &K, delta, e, &w);
            cs[0] = cs[0] + psl_s3_edge_rho(row, 1, &S, &Si, &K, delta, e, &w);
        }
        psl_lm_reduce<1, PSL_S3_NTERMS>(cs, s_red, flip);
        return cs[0];
    }
    __device__ __forceinline__ int classify(const PslS3& S, const PslS3& Si) {
        double cnt[1] = {0.0};
        for (int i = threadIdx.x; i < n; i += PSL_S3_BS) {
            if (out[i]) continue;
            if (psl_s3_pair_bad(P + PSL_S3_PAIR_FLOATS * i, &S, &Si, &K, th2)) {
                out[i] = 1;
                cnt[0] = cnt[0] + 1.0;
            }
        }
        psl_lm_reduce<1, PSL_S3_NTERMS>(cnt, s_red, flip);   // a count: exact in any order
        return (int)cnt[0];
    }
    __device__ __forceinline__ void call_done(int c, int its) {
        if (threadIdx.x == 0 && info) {
            info->calls = c + 1;
            info->iterations[c] = its;
        }
    }
};

// psl_lm_optimize<7> on a PslS3Vertex and psl_s3_rounds, written out for the kernel (the header says why).  A change to either is a
// change to the three functions below and the reverse.
// One trial step from the reduced sums: solves, guards the angle, applies the update as PslS3Vertex::candidate does.  Returns 1 and
// *Sn when there is a step to evaluate.
__device__ static inline int sim3_step(const double* acc, double lambda, const double* b, int fix_scale, const PslS3* S, double* x, PslS3* Sn,
                                       int* branches) {
    for (int j = 0; j < 7; ++j) x[j] = 0.0;
    int ok = psl_lm_solve<7>(acc, lambda, b, x);
    if (ok && !psl_lm_step_ok(x)) {   // a rotation angle outside the range of the restated sin / cos: as a failed solve
        ok = 0;
        for (int j = 0; j < 7; ++j) x[j] = 0.0;
    }
    *Sn = *S;
    if (ok) {
        if (fix_scale) x[6] = 0.0;
        int br = 0;
        psl_s3_oplus(x, fix_scale, S, g_s3_sctab, Sn, &br);
        *branches |= 1 << br;
    }
    return ok;
}

// one optimize(iterations) call on the estimate *T
__device__ static inline int sim3_optimize(Sim3DeviceSums& S, PslS3* T, int iterations, int fix_scale, int* branches) {
    int its = 0;
    double lambda = 0.0, ni = 2.0;
    int lm_bad = 0;
    for (int it = 0; it < iterations; ++it) {
        double acc[PSL_S3_NTERMS];
        PslS3 Ti;
        psl_s3_inverse(T, &Ti);
        S.system(*T, Ti, acc);
        double b[7];
        for (int j = 0; j < 7; ++j) b[j] = -acc[28 + j];
        double chi = acc[35];
        const double ini_chi = chi;
        if (it == 0) { lambda = psl_lm_lambda_init<7>(acc); ni = 2.0; lm_bad = 0; }
        double rho = 0.0;
        int qmax = 0;
        do {
            double x[7];
            PslS3 Tn;
            const int ok = sim3_step(acc, lambda, b, fix_scale, T, x, &Tn, branches);
            double temp_chi = PSL_LM_DBL_MAX;   // a failed solve (:120)
            if (ok) {
                PslS3 Tni;
                psl_s3_inverse(&Tn, &Tni);
                temp_chi = S.chi(Tn, Tni);
            }
            rho = psl_lm_rho<7>(chi, temp_chi, x, b, lambda);
            if (rho > 0 && __builtin_fabs(temp_chi) <= PSL_LM_DBL_MAX) {
                lambda = lambda * psl_lm_good_scale(rho);
                ni = 2.0;
                chi = temp_chi;
                *T = Tn;
            } else {
                lambda = lambda * ni;
                ni = ni * 2.0;
            }
            ++qmax;
        } while (rho < 0 && qmax < 10);
        ++its;
        if (qmax == 10 || rho == 0) break;                                 // Terminate
        if ((ini_chi - chi) * 1e3 < ini_chi) ++lm_bad; else lm_bad = 0;    // the _nBad rule
        if (lm_bad >= 3) break;
    }
    return its;
}

__device__ static inline int sim3_rounds(Sim3DeviceSums& S, const PslS3& S0, int npairs, int fix_scale, PslS3* S_out, int* written, int* branches) {
    *S_out = S0;
    *written = 0;
    *branches = 0;
    if (npairs <= 0) return 0;
    PslS3 T = S0, Ti;
    const int its0 = sim3_optimize(S, &T, 5, fix_scale, branches);
    S.call_done(0, its0);
    psl_s3_inverse(&T, &Ti);
    const int nbad = S.classify(T, Ti);
    const int more = nbad > 0 ? 10 : 5;
    if (npairs - nbad < 10) return 0;
    const int its1 = sim3_optimize(S, &T, more, fix_scale, branches);
    S.call_done(1, its1);
    psl_s3_inverse(&T, &Ti);
    const int nbad2 = S.classify(T, Ti);
    *S_out = T;
    *written = 1;
    return npairs - nbad - nbad2;
}

extern __shared__ float s_s3_pairs[];

__global__ __launch_bounds__(PSL_S3_BS) void k_sim3_optimize(Sim3Args A) {
    __shared__ double s_red[2 * 4 * PSL_S3_NTERMS];
    __shared__ PslS3 s_pert[PSL_S3_NPERT][2];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int n = A.npairs[c];
    PslS3 S0;
    {
        const PslSim3 in = A.Sin[c];
        psl_s3_from_rts(in.R, in.t, in.s, &S0);
    }
    PslSim3D* Sout = A.Sout + c;
    if (n <= 0 || n > A.pstride) {   // uniform: no pair (nothing to optimise), or a count the rows cannot hold or an error code
        if (tid == 0) {
            PslSim3D o;
            for (int i = 0; i < 4; ++i) o.q[i] = S0.q[i];
            for (int i = 0; i < 3; ++i) o.t[i] = S0.t[i];
            o.s = S0.s;
            *Sout = o;
            A.nin[c] = n < 0 ? PSLFE_E_INVALID : n > A.pstride ? PSLFE_E_CAPACITY : 0;
            if (A.info) {
                PslSim3Info I = {0, {0, 0}};
                A.info[c] = I;
            }
        }
        return;
    }
    const float* P = reinterpret_cast<const float*>(A.pairs + (size_t)c * A.pstride);
    uint8_t* out = A.bad + (size_t)c * A.pstride;
    for (int i = tid; i < n; i += PSL_S3_BS) out[i] = 0;   // the owner's bytes: every pair starts in the graph
    if (n <= A.lds_pairs) {
        for (int i = tid; i < n * PSL_S3_PAIR_FLOATS; i += PSL_S3_BS) s_s3_pairs[i] = P[i];
        P = s_s3_pairs;
        __syncthreads();
    }
    if (tid == 0 && A.info) {
        PslSim3Info I = {0, {0, 0}};
        A.info[c] = I;
    }
    Sim3DeviceSums S;
    S.P = P; S.out = out; S.n = n; S.K = A.K; S.th2 = A.th2; S.delta = A.delta; S.fix_scale = A.fix_scale;
    S.s_red = s_red; S.s_pert = s_pert; S.flip = 0; S.info = A.info ? A.info + c : nullptr;
    PslS3 T;
    int written = 0, branches = 0;
    const int nin = sim3_rounds(S, S0, n, A.fix_scale, &T, &written, &branches);
    if (tid == 0) {
        PslSim3D o;
        for (int i = 0; i < 4; ++i) o.q[i] = T.q[i];
        for (int i = 0; i < 3; ++i) o.t[i] = T.t[i];
        o.s = T.s;
        *Sout = o;
        A.nin[c] = nin;
        if (A.info) A.info[c].exp_branches = branches;
    }
}

// ---- the pairs of a candidate from its matches: the set-up loop src/Optimizer.cc:2854-2933 -------------------------------------------
// one row of a float 3x3 * 3x1 product plus a translation: a double sum in index order, rounded once (the convention above PslPose)
__device__ __forceinline__ float psl_s3_affine_row(const float* M, const float* X, float t) {
    double s = __dmul_rn((double)M[0], (double)X[0]);
    s = __dadd_rn(s, __dmul_rn((double)M[1], (double)X[1]));
    s = __dadd_rn(s, __dmul_rn((double)M[2], (double)X[2]));
    return (float)__dadd_rn(s, (double)t);
}

struct Sim3PairArgs {
    FrameStore S1, S2;
    int slot1;
    const int32_t* slots2;   // [ncand]
    int max_frames2;
    const int32_t* i2;       // [ncand][S1.cap]
    const PslMapPointGeom* mp1;
    const uint8_t* skip1;    // [n1]
    int n1;
    const PslMapPointGeom* mp2;   // [ncand][mp2stride]
    const uint8_t* skip2;
    int mp2stride;
    const PslPose* T1w;
    const PslPose* T2w;      // [ncand]
    float inv_sigma2[PSLFE_MAX_LEVELS];
    float sigma2[PSLFE_MAX_LEVELS];   // mvLevelSigma2, read only when sig is set
    int nlevels;
    PslSim3Pair* pairs;
    int32_t* pair_kp;
    int32_t* npairs;
    int pstride;
    float* sig;              // [ncand][pstride][2] or NULL: mvLevelSigma2 of the two octaves of each row (src/Sim3Solver.cc:84-85)
};

// one workgroup per candidate: KF1's keypoints in chunks of 256, compacted in keypoint order (psl_wg_compact of proj_kernels.h)
__global__ __launch_bounds__(256) void k_sim3_pairs(Sim3PairArgs A) {
    __shared__ int s_cnt[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int slot2 = A.slots2[c];
    if (slot2 < 0 || slot2 >= A.max_frames2) {   // uniform; a slot inside the store that was never set has meta.n == 0 since its creation
        if (tid == 0) A.npairs[c] = PSLFE_E_INVALID;
        return;
    }
    const int n = min(min(A.S1.meta[A.slot1].n, A.S1.cap), A.n1);
    const int n2 = min(min(A.S2.meta[slot2].n, A.S2.cap), A.mp2stride);
    const PslKeyPoint* kps1 = A.S1.kps + (size_t)A.slot1 * A.S1.cap;
    const PslKeyPoint* kps2 = A.S2.kps + (size_t)slot2 * A.S2.cap;
    const int32_t* i2s = A.i2 + (size_t)c * A.S1.cap;
    const PslMapPointGeom* mp2 = A.mp2 + (size_t)c * A.mp2stride;
    const uint8_t* skip2 = A.skip2 + (size_t)c * A.mp2stride;
    PslSim3Pair* pairs = A.pairs + (size_t)c * A.pstride;
    int32_t* pair_kp = A.pair_kp ? A.pair_kp + (size_t)c * A.pstride : nullptr;
    const PslPose T1 = A.T1w[0], T2 = A.T2w[c];
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {   // uniform
        const int i = i0 + tid;
        int j = -1;
        if (i < n) {
            j = i2s[i];                                     // vpMatches1[i] == NULL, or i2 < 0 (:2856, :2869)
            if (j < 0 || j >= n2) j = -1;                   // an index outside its array drops the pair
            else if (A.skip1[i] || skip2[j]) j = -1;        // pMP1 NULL or bad, pMP2 bad (:2867-2869)
        }
        int kept;
        const int pos = base + psl_wg_compact<256>(j >= 0, s_cnt, &kept);
        base += kept;
        if (j >= 0 && pos < A.pstride) {
            const PslKeyPoint k1 = kps1[i], k2 = kps2[j];
            const float X1[3] = {A.mp1[i].x, A.mp1[i].y, A.mp1[i].z}, X2[3] = {mp2[j].x, mp2[j].y, mp2[j].z};
            PslSim3Pair p;
            p.u1 = k1.x; p.v1 = k1.y; p.inv_sigma2_1 = A.inv_sigma2[min(max(k1.octave, 0), A.nlevels - 1)];
            p.u2 = k2.x; p.v2 = k2.y; p.inv_sigma2_2 = A.inv_sigma2[min(max(k2.octave, 0), A.nlevels - 1)];
            for (int r = 0; r < 3; ++r) {
                p.P1c[r] = psl_s3_affine_row(T1.R + 3 * r, X1, T1.t[r]);   // P3D1c = R1w*P3D1w + t1w (:2873)
                p.P2c[r] = psl_s3_affine_row(T2.R + 3 * r, X2, T2.t[r]);   // P3D2c = R2w*P3D2w + t2w (:2881)
            }
            pairs[pos] = p;
            if (pair_kp) pair_kp[pos] = i;
            if (A.sig) {
                float* sg = A.sig + 2 * ((size_t)c * A.pstride + pos);
                sg[0] = A.sigma2[min(max(k1.octave, 0), A.nlevels - 1)];
                sg[1] = A.sigma2[min(max(k2.octave, 0), A.nlevels - 1)];
            }
        }
    }
    if (tid == 0) A.npairs[c] = base;
}

namespace {

int sim3_launch(pslfe_ctx* ctx, int ncand, const PslSim3* d_S12_in, const PslSim3Pair* d_pairs, const int32_t* d_npairs, int pstride,
                const PslCamera* cam1, const PslCamera* cam2, float th2, int fix_scale, PslSim3D* d_S12_out, uint8_t* d_bad, int32_t* d_nin,
                PslSim3Info* d_info) {
    Sim3Args A;
    A.Sin = d_S12_in; A.pairs = d_pairs; A.npairs = d_npairs; A.pstride = pstride;
    A.lds_pairs = pstride < PSL_S3_LDS_PAIRS ? pstride : PSL_S3_LDS_PAIRS;
    A.K.fx1 = (double)cam1->fx; A.K.fy1 = (double)cam1->fy; A.K.cx1 = (double)cam1->cx; A.K.cy1 = (double)cam1->cy;
    A.K.fx2 = (double)cam2->fx; A.K.fy2 = (double)cam2->fy; A.K.cx2 = (double)cam2->cx; A.K.cy2 = (double)cam2->cy;
    A.th2 = (double)th2; A.delta = PSL_S3_HUBER_DELTA(th2); A.fix_scale = fix_scale ? 1 : 0;
    A.Sout = d_S12_out; A.bad = d_bad; A.nin = d_nin; A.info = d_info;
    const size_t lds = (size_t)A.lds_pairs * sizeof(PslSim3Pair);
    {
        PSL_STAGE_BEGIN(ctx, "sim3.optimize");
        k_sim3_optimize<<<ncand, PSL_S3_BS, lds, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "sim3.optimize");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

// both set-up entry points; level_sigma2 / d_sigma2 are NULL for the first
int sim3_pairs(pslfe_frame* f1, int slot1, pslfe_frame* f2, const int32_t* d_slots2, int ncand, const int32_t* d_i2, const PslMapPointGeom* d_mp1,
               const uint8_t* d_skip1, int n1, const PslMapPointGeom* d_mp2, const uint8_t* d_skip2, int mp2stride, const PslPose* d_T1w,
               const PslPose* d_T2w, const float* inv_level_sigma2, int nlevels, PslSim3Pair* d_pairs, int32_t* d_pair_kp, int32_t* d_npairs,
               int pstride, const float* level_sigma2, float* d_sigma2, const char* who) {
    PSL_REQUIRE(ncand >= 0 && n1 >= 0 && mp2stride >= 0 && pstride >= 0, PSLFE_E_INVALID, "%s: ncand = %d, n1 = %d, mp2stride = %d, pstride = %d",
                who, ncand, n1, mp2stride, pstride);
    if (ncand == 0) return PSLFE_OK;
    PSL_REQUIRE(f1 && f2, PSLFE_E_INVALID, "%s: NULL frame store", who);
    PSL_REQUIRE(f1->ctx == f2->ctx, PSLFE_E_INVALID, "%s: the frame stores belong to different contexts", who);
    PSL_REQUIRE(slot1 >= 0 && slot1 < f1->max_frames, PSLFE_E_INVALID, "%s: slot %d of %d", who, slot1, f1->max_frames);
    PSL_REQUIRE(f1->slot_set[slot1], PSLFE_E_STATE, "%s: slot %d not set", who, slot1);
    PSL_REQUIRE(nlevels >= 1 && nlevels <= PSLFE_MAX_LEVELS && inv_level_sigma2, PSLFE_E_INVALID, "%s: nlevels = %d (1..%d) or NULL table", who,
                nlevels, PSLFE_MAX_LEVELS);
    PSL_REQUIRE(d_slots2 && d_i2 && d_T1w && d_T2w && d_npairs, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(n1 == 0 || (d_mp1 && d_skip1), PSLFE_E_INVALID, "%s: NULL map points with n1 = %d", who, n1);
    PSL_REQUIRE(mp2stride == 0 || (d_mp2 && d_skip2), PSLFE_E_INVALID, "%s: NULL map points with mp2stride = %d", who, mp2stride);
    PSL_REQUIRE(pstride == 0 || d_pairs, PSLFE_E_INVALID, "%s: NULL pairs with pstride = %d", who, pstride);
    PSL_REQUIRE(!d_sigma2 || level_sigma2, PSLFE_E_INVALID, "%s: NULL table of level sigma2", who);
    pslfe_ctx* ctx = f1->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    Sim3PairArgs A;
    A.S1 = f1->S; A.S2 = f2->S; A.slot1 = slot1; A.slots2 = d_slots2; A.max_frames2 = f2->max_frames; A.i2 = d_i2;
    A.mp1 = d_mp1; A.skip1 = d_skip1; A.n1 = n1; A.mp2 = d_mp2; A.skip2 = d_skip2; A.mp2stride = mp2stride;
    A.T1w = d_T1w; A.T2w = d_T2w; A.nlevels = nlevels;
    for (int l = 0; l < PSLFE_MAX_LEVELS; ++l) A.inv_sigma2[l] = l < nlevels ? inv_level_sigma2[l] : 0.f;
    for (int l = 0; l < PSLFE_MAX_LEVELS; ++l) A.sigma2[l] = d_sigma2 && l < nlevels ? level_sigma2[l] : 0.f;
    A.pairs = d_pairs; A.pair_kp = d_pair_kp; A.npairs = d_npairs; A.pstride = pstride; A.sig = d_sigma2;
    {
        PSL_STAGE_BEGIN(ctx, "sim3.pairs");
        k_sim3_pairs<<<ncand, 256, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "sim3.pairs");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_sim3_optimize_device(pslfe_ctx* ctx, int ncand, const PslSim3* d_S12_in, const PslSim3Pair* d_pairs, const int32_t* d_npairs,
                               int pstride, const PslCamera* cam1, const PslCamera* cam2, float th2, int fix_scale, PslSim3D* d_S12_out,
                               uint8_t* d_bad, int32_t* d_nin, PslSim3Info* d_info) {
    static const char* who = "pslfe_sim3_optimize_device";
    PSL_REQUIRE(ncand >= 0 && pstride >= 0, PSLFE_E_INVALID, "%s: ncand = %d, pstride = %d", who, ncand, pstride);
    if (ncand == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && cam1 && cam2, PSLFE_E_INVALID, "%s: NULL context or camera", who);
    PSL_REQUIRE(d_S12_in && d_npairs && d_S12_out && d_nin, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(pstride == 0 || (d_pairs && d_bad), PSLFE_E_INVALID, "%s: NULL pairs or outlier bytes with pstride = %d", who, pstride);
    PSL_HIP(hipSetDevice(ctx->device));
    return sim3_launch(ctx, ncand, d_S12_in, d_pairs, d_npairs, pstride, cam1, cam2, th2, fix_scale, d_S12_out, d_bad, d_nin, d_info);
}

int pslfe_sim3_optimize(pslfe_ctx* ctx, const PslSim3* S12, const PslSim3Pair* pairs, int npairs, const PslCamera* cam1, const PslCamera* cam2,
                        float th2, int fix_scale, PslSim3D* S12_out, uint8_t* bad, int* nin) {
    static const char* who = "pslfe_sim3_optimize";
    PSL_REQUIRE(npairs >= 0, PSLFE_E_INVALID, "%s: npairs = %d", who, npairs);
    PSL_REQUIRE(ctx && cam1 && cam2 && S12 && S12_out && nin, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(npairs == 0 || (pairs && bad), PSLFE_E_INVALID, "%s: NULL pairs or outlier bytes with npairs = %d", who, npairs);
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int32_t n32 = npairs;
    const PslSim3* d_S = psl_scratch_up(ctx, S12, 1, st, &e);
    const PslSim3Pair* d_pairs = psl_scratch_up(ctx, npairs ? pairs : nullptr, (size_t)npairs, st, &e);
    const int32_t* d_n = psl_scratch_up(ctx, &n32, 1, st, &e);
    PslSim3D* d_out = psl_scratch_up(ctx, (const PslSim3D*)nullptr, 1, st, &e);
    uint8_t* d_bad = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)npairs, st, &e);
    int32_t* d_nin = psl_scratch_up(ctx, (const int32_t*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    if (int rc = sim3_launch(ctx, 1, d_S, d_pairs, d_n, npairs, cam1, cam2, th2, fix_scale, d_out, d_bad, d_nin, nullptr)) return rc;
    int32_t ni = 0;
    PSL_HIP(hipMemcpyAsync(S12_out, d_out, sizeof(PslSim3D), hipMemcpyDeviceToHost, st));
    if (npairs) PSL_HIP(hipMemcpyAsync(bad, d_bad, (size_t)npairs, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(&ni, d_nin, sizeof(ni), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *nin = ni;
    return PSLFE_OK;
}

int pslfe_sim3_pairs_from_matches_device(pslfe_frame* f1, int slot1, pslfe_frame* f2, const int32_t* d_slots2, int ncand, const int32_t* d_i2,
                                         const PslMapPointGeom* d_mp1, const uint8_t* d_skip1, int n1, const PslMapPointGeom* d_mp2,
                                         const uint8_t* d_skip2, int mp2stride, const PslPose* d_T1w, const PslPose* d_T2w,
                                         const float* inv_level_sigma2, int nlevels, PslSim3Pair* d_pairs, int32_t* d_pair_kp,
                                         int32_t* d_npairs, int pstride) {
    return sim3_pairs(f1, slot1, f2, d_slots2, ncand, d_i2, d_mp1, d_skip1, n1, d_mp2, d_skip2, mp2stride, d_T1w, d_T2w, inv_level_sigma2, nlevels,
                      d_pairs, d_pair_kp, d_npairs, pstride, nullptr, nullptr, "pslfe_sim3_pairs_from_matches_device");
}

int pslfe_sim3_pairs_sigma2_from_matches_device(pslfe_frame* f1, int slot1, pslfe_frame* f2, const int32_t* d_slots2, int ncand,
                                                const int32_t* d_i2, const PslMapPointGeom* d_mp1, const uint8_t* d_skip1, int n1,
                                                const PslMapPointGeom* d_mp2, const uint8_t* d_skip2, int mp2stride, const PslPose* d_T1w,
                                                const PslPose* d_T2w, const float* inv_level_sigma2, int nlevels, PslSim3Pair* d_pairs,
                                                int32_t* d_pair_kp, int32_t* d_npairs, int pstride, const float* level_sigma2,
                                                float* d_sigma2) {
    return sim3_pairs(f1, slot1, f2, d_slots2, ncand, d_i2, d_mp1, d_skip1, n1, d_mp2, d_skip2, mp2stride, d_T1w, d_T2w, inv_level_sigma2, nlevels,
                      d_pairs, d_pair_kp, d_npairs, pstride, level_sigma2, d_sigma2, "pslfe_sim3_pairs_sigma2_from_matches_device");
}

}  // extern "C"
