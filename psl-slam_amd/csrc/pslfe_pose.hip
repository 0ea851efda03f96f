// libpslfe: Optimizer::PoseOptimization (src/Optimizer.cc:239-1023), its point edges and its LIL edges, for K frames in one launch.
// Product code.
// Reference behaviour restated (in double, in the reference's order of decisions):
//   edge set-up, the four rounds, the classification after a round   src/Optimizer.cc:282-363, :696-780, :1011-1022
//   one iteration: lambda, trials, rho, Terminate                    Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   the iteration loop of a round                                    Thirdparty/g2o/g2o/core/sparse_optimizer.cpp:354-419
//   the LIL edges: set-up, error / Jacobian, classification            src/Optimizer.cc:619-694, add_inc/EdgeLIL.h:210-439, :973-1008
// Who owns what.  pose_kernels.h holds the arithmetic of an edge, the update and the four rounds psl_po_rounds; lm_kernels.h holds
// the solve, the Huber kernel and the Levenberg driver psl_lm_levenberg (the iterations and trials of a round with every decision
// between two sums), which OptimizeSim3, the local bundle adjustment and the essential graph share.  The host loop of
// tools/dropin/pose_main.cpp instantiates psl_po_rounds and with it psl_lm_optimize<6>, the driver on one vertex.  k_pose_optimize
// calls the same primitives but keeps the rounds and the driver's loop written out in its body: instantiating the driver here gave
// the same registers, LDS and scratch and the same per-edge and reduction code, but launches 0.6 to 1.9 % slower than this form on
// an MI355X (profiles/pose_driver_ab.json).  So the loop has three texts that are changed together: the driver
// psl_lm_levenberg, and the two loops written out here and in k_sim3_optimize; a change to psl_po_rounds is likewise a change to
// the loop below and the reverse.  tests/test_pose_*_gpu.py compare both with the numpy restatement bit for bit.  The device's own: which thread owns which edge, the order of the sums (its steps 2 and 3 are
// psl_lm_reduce of lm_device.h, shared with pslfe_sim3.hip), the LDS copy of the rows, the early return, the edge set-up kernels.
// Scope: the monocular and stereo point edges (k_pose_optimize<false>, what pslfe_pose_optimize[_device] launch) and, in
// k_pose_optimize<true> (pslfe_pose_optimize_lil[_device]), the LIL edges (EdgeLILSE3ProjectXYZ with its fixed VertexLIL) as well.
// The LIL edges of a frame extend its edge index space: LIL edge j has the index n + j (g2o adds them after the point edges), so
// ownership (index mod 256) and the order of the sums stay a function of the edge index and the counts alone.  Their rows (23
// doubles) are read from HBM; a LIL edge adds its 28 terms row by row (psl_po_lil_add_terms), so that no 6x6 Jacobian is live next
// to the accumulators (no scratch in either instantiation: profiles/pose_lil_codegen.txt).  The `< 3` and `< 10` rules count both
// kinds; the return value counts an outlying LIL edge as good (:1022).  Two oddities of the reference are kept:
// the Jacobian's row 2 at line 2's end point (EdgeLIL.h:273-275) and mvle_l[i] indexed by the plane (src/Optimizer.cc:658).
// Conventions: include/pslfe.h above pslfe_pose_optimize_device.
//
// Layout.  One workgroup of 256 threads per frame, resident through every round, iteration and trial; there is no launch per
// iteration.  The edge rows (7 floats) of a frame with at most PSL_POSE_LDS_EDGES edges are copied to LDS once and read from there
// (row stride 7 words: consecutive rows fall into different banks); a larger frame reads them from HBM, with the same arithmetic.
// Thread t owns the edges t, t + 256, t + 512, ...: it computes their error, Jacobian and 28 terms, and it alone reads and writes their
// outlier bytes, which are the edge levels of the next round.
//
// Order of the sums.  H (21 values), b (6) and the robust chi2 of the active edges are summed in an order fixed by the edge index
// and the edge count n alone:
//   1. partial sum p (0 <= p < 256) starts at +0.0 and adds the terms of the active edges p, p + 256, p + 512, ... in ascending order;
//   2. inside each group of 64 consecutive partial sums, for s = 32, 16, 8, 4, 2, 1: partial[g*64 + l] += partial[g*64 + l + s]
//      for l < s; the group's sum is partial[g*64];
//   3. the four group sums are added as ((G0 + G1) + G2) + G3.
// Step 1 runs in a thread, step 2 with cross-lane operations inside a wave, step 3 through LDS (one barrier per reduction: the four
// wave sums alternate between two LDS buffers).  The block size is fixed, so nothing depends on the launch geometry, the batch size
// or the frame's position in the batch.  tests/pose_opt_cases.py implements the same order in numpy and reproduces the bits.
//
// Solve and update.  Every lane of every wave solves the 6x6 system (LDLt without pivoting, psl_lm_solve<6>) and applies the SE3
// update from the reduced sums it has read from LDS.  The inputs are the same bits in every lane and every operation is a single
// IEEE operation, so the lanes agree bit for bit and all control flow is uniform.  One lane with a broadcast would execute the
// same number of wave instructions (a wave issues for 64 lanes whether one or all are live) and add an LDS round trip and a barrier
// per trial; the redundant form needs neither.  "The solve failed" (a pivot that is not a finite positive number) makes the trial's
// chi2 DBL_MAX, as g2o does for a failed LDLT, with a zero step in the rho formula; the trial is rejected and lambda grows.
// A step whose rotation angle |omega| is not below 105414350 (the range of the restated sin / cos; NaN included) is treated the same way.
// A frame with few edges runs on the same 256 threads; waves without edges only take part in the barriers.
// sin / cos of the rotation angle are psl_glibc_sin / psl_glibc_cos (psl_sincos_glibc.h), bit-identical to glibc; no device math
// library call is made.
#include <string.h>

#include "pslfe_internal.h"
#include "match_kernels.h"
#include "proj_kernels.h"
#include "pose_kernels.h"
#include "lm_device.h"

#define PSL_POSE_BS PSL_LM_LANES
#define PSL_POSE_LDS_EDGES 2048   // 56 KB of edge rows

static_assert(sizeof(PslPoseLilEdge) == PSL_POSE_LIL_DOUBLES * sizeof(double), "a LIL row is 23 doubles");
static_assert(sizeof(PslPoseEdge) == 28 && sizeof(PslPoseInfo) == 20 && sizeof(PslPose) == 48, "pose PODs");
static_assert(PSL_POSE_BS == 4 * PSL_LM_GROUP, "four waves of 64");

__device__ const double g_pose_sctab[444] = {
#include "psl_sincostab.inc"
};

struct PoseArgs {
    const PslPose* Tin;
    const PslPoseEdge* edges;
    const int32_t* nedges;
    int estride, lds_edges;
    PslPoseCamD K;
    PslPose* Tout;
    uint8_t* outlier;
    int32_t* ngood;
    PslPoseInfo* info;
};
// the LIL edges of the frames (k_pose_optimize<true> only): rows of 23 doubles read from HBM, LIL edge j has the edge index n + j
struct PoseLilArgs {
    const PslPoseLilEdge* lil;
    const int32_t* nlil;
    int lstride;
    uint8_t* outlier;
};

extern __shared__ float s_pose_edges[];

// LIL: the frames have LIL edges (B); without them B is not read and the kernel is the point-edge kernel.  n: the point edges, m: the
// LIL edges, nt = n + m: the edges (the `< 3` and `< 10` rules and the order of the sums see one index space, points first).
// The loops over r, it and the trials are psl_po_rounds and psl_lm_optimize<6> written out (the header says why).
template <bool LIL>
__global__ __launch_bounds__(PSL_POSE_BS) void k_pose_optimize(PoseArgs A, PoseLilArgs B) {
    __shared__ double s_red[2 * 4 * PSL_POSE_NTERMS];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int n = A.nedges[f];
    const int m = LIL ? B.nlil[f] : 0;
    const int nt = n + m;
    const float* Tin = reinterpret_cast<const float*>(A.Tin + f);
    float* Tout = reinterpret_cast<float*>(A.Tout + f);
    const bool over = n > A.estride || (LIL && m > B.lstride);
    const bool negative = LIL && (n < 0 || m < 0);   // a negative count, such as an error code pslfe_pose_lil_edges_device left in d_nlil
    if (nt < 3 || over || negative) {   // uniform: fewer than 3 edges (src/Optimizer.cc:696), or a count the rows cannot hold
        if (tid == 0) {
            float P[12];
            for (int i = 0; i < 12; ++i) P[i] = Tin[i];
            for (int i = 0; i < 12; ++i) Tout[i] = P[i];
            A.ngood[f] = negative ? PSLFE_E_INVALID : over ? PSLFE_E_CAPACITY : 0;
            if (A.info) {
                PslPoseInfo I = {0, {0, 0, 0, 0}};
                A.info[f] = I;
            }
        }
        return;
    }
    const float* E = reinterpret_cast<const float*>(A.edges + (size_t)f * A.estride);
    if (n <= A.lds_edges) {
        for (int i = tid; i < n * 7; i += PSL_POSE_BS) s_pose_edges[i] = E[i];
        E = s_pose_edges;
        __syncthreads();
    }
    uint8_t* out = A.outlier + (size_t)f * A.estride;
    // the first LIL edge of this thread: the smallest j with (n + j) mod 256 == tid
    const int j0 = LIL ? ((tid - n % PSL_POSE_BS) + PSL_POSE_BS) % PSL_POSE_BS : 0;
    const double* Lrows = LIL ? reinterpret_cast<const double*>(B.lil + (size_t)f * B.lstride) : nullptr;
    uint8_t* out_lil = LIL ? B.outlier + (size_t)f * B.lstride : nullptr;
    const PslPoseCamD K = A.K;
    PslSE3 T0;
    {
        float P[12];
        for (int i = 0; i < 12; ++i) P[i] = Tin[i];
        psl_po_from_pose(P, P + 9, &T0);
    }
    if (tid == 0 && A.info) {
        PslPoseInfo I = {0, {0, 0, 0, 0}};
        A.info[f] = I;
    }
    int flip = 0, nbad = 0, nbad_lil = 0;
    PslSE3 T = T0;
    for (int r = 0; r < 4; ++r) {
        T = T0;                       // vSE3->setEstimate(Converter::toSE3Quat(pFrame->mTcw)) (:719)
        const bool robust = r < 3;    // e->setRobustKernel(0) after round index 2 (:749)
        int its = 0;
        if (nt - nbad - nbad_lil > 0) {   // without an active edge g2o has no vertex to optimise and optimize() returns at once
            double lambda = 0.0, ni = 2.0;
            int lm_bad = 0;
            for (int it = 0; it < 10; ++it) {
                double acc[PSL_POSE_NTERMS];
#pragma unroll
                for (int k = 0; k < PSL_POSE_NTERMS; ++k) acc[k] = 0.0;
                for (int i = tid; i < n; i += PSL_POSE_BS) {
                    if (r > 0 && out[i]) continue;
                    double e[3], Pc[3], rho0, rho1 = 1.0;
                    const int mono = psl_po_error(E + 7 * i, &T, &K, e, Pc);
                    const double is2 = (double)E[7 * i + 3];
                    const double c = psl_po_chi2(e, is2, mono);
                    rho0 = c;
                    if (robust) psl_lm_huber(c, PSL_POSE_DELTA(mono), &rho0, &rho1);
                    psl_po_add_terms(e, Pc, mono, is2, rho0, rho1, &K, acc);
                }
                if constexpr (LIL) {
                    for (int j = j0; j < m; j += PSL_POSE_BS) {
                        if (r > 0 && out_lil[j]) continue;
                        const double* L = Lrows + (size_t)j * PSL_POSE_LIL_DOUBLES;
                        double e[6], rho0, rho1 = 1.0;
                        psl_po_lil_error(L, &T, &K, e);
                        const double c = psl_po_lil_chi2(e);
                        rho0 = c;
                        if (robust) psl_lm_huber(c, PSL_POSE_DELTA_LIL, &rho0, &rho1);
                        psl_po_lil_add_terms(L, e, &T, rho0, rho1, &K, acc);
                    }
                }
                psl_lm_reduce<PSL_POSE_NTERMS, PSL_POSE_NTERMS>(acc, s_red, flip);
                double b[6];
#pragma unroll
                for (int j = 0; j < 6; ++j) b[j] = -acc[21 + j];
                double chi = acc[27];
                const double ini_chi = chi;
                if (it == 0) { lambda = psl_lm_lambda_init<6>(acc); ni = 2.0; lm_bad = 0; }
                double rho = 0.0;
                int qmax = 0;
                do {
                    double x[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                    int ok = psl_lm_solve<6>(acc, lambda, b, x);
                    if (ok && !psl_lm_step_ok(x)) {   // a rotation angle outside the range of the restated sin / cos: as a failed solve
                        ok = 0;
#pragma unroll
                        for (int j = 0; j < 6; ++j) x[j] = 0.0;
                    }
                    double temp_chi = PSL_LM_DBL_MAX;   // a failed solve (:120)
                    PslSE3 Tn = T;
                    if (ok) {
                        PslSE3 dT;
                        psl_po_exp(x, &dT, g_pose_sctab);
                        psl_po_mul(&dT, &T, &Tn);          // oplusImpl: exp(update) * estimate
                        double cs[1] = {0.0};
                        for (int i = tid; i < n; i += PSL_POSE_BS) {
                            if (r > 0 && out[i]) continue;
                            double e[3], Pc[3], rho0, rho1 = 1.0;
                            const int mono = psl_po_error(E + 7 * i, &Tn, &K, e, Pc);
                            const double c = psl_po_chi2(e, (double)E[7 * i + 3], mono);
                            rho0 = c;
                            if (robust) psl_lm_huber(c, PSL_POSE_DELTA(mono), &rho0, &rho1);
                            cs[0] = cs[0] + rho0;
                        }
                        if constexpr (LIL) {
                            for (int j = j0; j < m; j += PSL_POSE_BS) {
                                if (r > 0 && out_lil[j]) continue;
                                double e[6], rho0, rho1 = 1.0;
                                psl_po_lil_error(Lrows + (size_t)j * PSL_POSE_LIL_DOUBLES, &Tn, &K, e);
                                const double c = psl_po_lil_chi2(e);
                                rho0 = c;
                                if (robust) psl_lm_huber(c, PSL_POSE_DELTA_LIL, &rho0, &rho1);
                                cs[0] = cs[0] + rho0;
                            }
                        }
                        psl_lm_reduce<1, PSL_POSE_NTERMS>(cs, s_red, flip);
                        temp_chi = cs[0];
                    }
                    rho = psl_lm_rho<6>(chi, temp_chi, x, b, lambda);
                    if (rho > 0 && __builtin_fabs(temp_chi) <= PSL_LM_DBL_MAX) {
                        lambda = lambda * psl_lm_good_scale(rho);
                        ni = 2.0;
                        chi = temp_chi;
                        T = Tn;
                    } else {
                        lambda = lambda * ni;
                        ni = ni * 2.0;
                    }
                    ++qmax;
                } while (rho < 0 && qmax < 10);
                ++its;
                if (qmax == 10 || rho == 0) break;                                  // Terminate
                if ((ini_chi - chi) * 1e3 < ini_chi) ++lm_bad; else lm_bad = 0;     // the _nBad rule
                if (lm_bad >= 3) break;
            }
        }
        // the plain chi2 of every edge at the round's pose, as a float, against 5.991f / 7.815f (:724-780)
        // and of every LIL edge against 11.07f (:977-1008); nBad counts the point edges only
        double cnt[LIL ? 2 : 1] = {0.0};
        for (int i = tid; i < n; i += PSL_POSE_BS) {
            double e[3], Pc[3];
            const int mono = psl_po_error(E + 7 * i, &T, &K, e, Pc);
            const float c = (float)psl_po_chi2(e, (double)E[7 * i + 3], mono);
            const bool bad = c > (mono ? 5.991f : 7.815f);
            out[i] = bad ? 1 : 0;
            cnt[0] = cnt[0] + (bad ? 1.0 : 0.0);
        }
        if constexpr (LIL) {
            for (int j = j0; j < m; j += PSL_POSE_BS) {
                double e[6];
                psl_po_lil_error(Lrows + (size_t)j * PSL_POSE_LIL_DOUBLES, &T, &K, e);
                const bool bad = (float)psl_po_lil_chi2(e) > 11.07f;
                out_lil[j] = bad ? 1 : 0;
                cnt[1] = cnt[1] + (bad ? 1.0 : 0.0);
            }
        }
        psl_lm_reduce<LIL ? 2 : 1, PSL_POSE_NTERMS>(cnt, s_red, flip);   // counts: exact in any order
        nbad = (int)cnt[0];
        if constexpr (LIL) nbad_lil = (int)cnt[1];
        if (tid == 0 && A.info) {
            A.info[f].rounds = r + 1;
            A.info[f].iterations[r] = its;
        }
        if (nt < 10) break;   // optimizer.edges().size() < 10: all edges, not the active ones (:1011)
    }
    if (tid == 0) {
        float P[12];
        psl_po_to_pose(&T, P, P + 9);
        for (int i = 0; i < 12; ++i) Tout[i] = P[i];
        A.ngood[f] = nt - nbad;   // nInitialCorrespondences - nBad (:1022): an outlying LIL edge still counts as good
    }
}

// ---- the edges of a frame from its matches ------------------------------------------------------------------------------------------
struct PoseEdgeArgs {
    FrameStore S;
    int slot0;
    const int32_t* mp_index;   // [nframes][S.cap]
    const PslMapPointGeom* mp;
    int mpstride;
    float inv_sigma2[PSLFE_MAX_LEVELS];
    int nlevels;
    PslPoseEdge* edges;
    int32_t* edge_kp;
    int32_t* nedges;
    int estride;
};

// one workgroup per frame: the keypoints in chunks of 256, compacted in keypoint order (psl_wg_compact of proj_kernels.h: a ballot
// inside the wave and a scan of the four wave counts)
__global__ __launch_bounds__(256) void k_pose_edges(PoseEdgeArgs A) {
    __shared__ int s_cnt[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    const int slot = A.slot0 + f;
    const int n = min(A.S.meta[slot].n, A.S.cap);
    const PslKeyPoint* kps = A.S.kps + (size_t)slot * A.S.cap;
    const float* uright = A.S.uright + (size_t)slot * A.S.cap;
    const int32_t* idx = A.mp_index + (size_t)f * A.S.cap;
    const PslMapPointGeom* mp = A.mp + (size_t)f * A.mpstride;
    PslPoseEdge* edges = A.edges + (size_t)f * A.estride;
    int32_t* edge_kp = A.edge_kp ? A.edge_kp + (size_t)f * A.estride : nullptr;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {   // uniform
        const int i = i0 + tid;
        int m = -1;
        if (i < n) {
            m = idx[i];
            if (m < 0 || m >= A.mpstride) m = -1;
        }
        int kept;
        const int pos = base + psl_wg_compact<256>(m >= 0, s_cnt, &kept);
        base += kept;
        if (m >= 0 && pos < A.estride) {
            const PslKeyPoint kp = kps[i];
            const int oct = min(max(kp.octave, 0), A.nlevels - 1);
            PslPoseEdge e;
            e.u = kp.x; e.v = kp.y; e.ur = uright[i]; e.inv_sigma2 = A.inv_sigma2[oct];
            e.x = mp[m].x; e.y = mp[m].y; e.z = mp[m].z;
            edges[pos] = e;
            if (edge_kp) edge_kp[pos] = i;
        }
    }
    if (tid == 0) A.nedges[f] = base;
}

// ---- mvpMapPoints of a frame from the rows of a window search ------------------------------------------------------------------------
// one workgroup per frame: every keypoint -1; the last row (in row order, as F.mvpMapPoints[bestIdx] = pMP overwrites) that matched a
// keypoint leaves its row number there; the row number is replaced by the row's owner
__global__ __launch_bounds__(256) void k_pose_mp_index(const int32_t* __restrict__ match, const int32_t* __restrict__ owner,
                                                       const int32_t* __restrict__ nq, int qstride, int cap, int32_t* __restrict__ mp_index) {
    const int f = blockIdx.x, tid = threadIdx.x;
    int32_t* idx = mp_index + (size_t)f * cap;
    const int32_t* m = match + (size_t)f * qstride;
    const int32_t* ow = owner + (size_t)f * qstride;
    const int n = min(max(nq[f], 0), qstride);
    for (int i = tid; i < cap; i += 256) idx[i] = -1;
    __syncthreads();
    for (int q = tid; q < n; q += 256) {
        const int kp = m[q];
        if (kp >= 0 && kp < cap) atomicMax(&idx[kp], q);
    }
    __syncthreads();
    for (int i = tid; i < cap; i += 256) {
        const int q = idx[i];
        if (q >= 0) idx[i] = ow[q];
    }
}

// ---- the LIL edges of a frame from its planes: the set-up loop src/Optimizer.cc:631-693 ---------------------------------------------------
struct PoseLilEdgeArgs {
    const double* le_l;        // [nframes][le_stride][6]     mvle_l, one row per crossing
    const double* cross2d;     // [nframes][plane_stride][2]  CrossPoint_2D, one row per plane
    const int32_t* nplanes;    // [nframes]
    const int32_t* lil_index;  // [nframes][plane_stride]
    const PslMapLil* map;
    int le_stride, plane_stride, nmap;
    PslPoseLilEdge* lil;
    int32_t* edge_plane;
    int32_t* nlil;
    int lstride;
};

// one workgroup per frame: the planes in chunks of 256, compacted in plane order as k_pose_edges compacts the keypoints.  Plane i
// takes row i of mvle_l and row i of CrossPoint_2D, as the reference does (:658-660).
__global__ __launch_bounds__(256) void k_pose_lil_edges(PoseLilEdgeArgs A) {
    __shared__ int s_cnt[4];
    const int f = blockIdx.x, tid = threadIdx.x;
    if (A.nplanes[f] > min(A.plane_stride, A.le_stride)) {   // uniform: planes the rows cannot hold are reported, not dropped
        if (tid == 0) A.nlil[f] = PSLFE_E_CAPACITY;
        return;
    }
    const int n = A.nplanes[f];
    const double* le = A.le_l + (size_t)f * A.le_stride * 6;
    const double* c2 = A.cross2d + (size_t)f * A.plane_stride * 2;
    const int32_t* idx = A.lil_index + (size_t)f * A.plane_stride;
    PslPoseLilEdge* lil = A.lil + (size_t)f * A.lstride;
    int32_t* edge_plane = A.edge_plane ? A.edge_plane + (size_t)f * A.lstride : nullptr;
    int base = 0;
    for (int i0 = 0; i0 < n; i0 += 256) {   // uniform
        const int i = i0 + tid;
        int q = -1;
        if (i < n) {
            q = idx[i];
            if (q < 0 || q >= A.nmap) q = -1;          // mvpMapInsecs[i] == NULL
            else if (A.map[q].bad) q = -1;             // mbBad (:634)
        }
        int kept;
        const int pos = base + psl_wg_compact<256>(q >= 0, s_cnt, &kept);
        base += kept;
        if (q >= 0 && pos < A.lstride) {
            PslPoseLilEdge e;
            const double* W = A.map[q].w;
            for (int k = 0; k < 6; ++k) { e.line1[k] = W[k]; e.line2[k] = W[6 + k]; }
            for (int k = 0; k < 3; ++k) { e.cross[k] = W[12 + k]; e.obs1[k] = le[6 * (size_t)i + k]; e.obs2[k] = le[6 * (size_t)i + 3 + k]; }
            e.obs_ins[0] = c2[2 * (size_t)i]; e.obs_ins[1] = c2[2 * (size_t)i + 1];
            lil[pos] = e;
            if (edge_plane) edge_plane[pos] = i;
        }
    }
    if (tid == 0) A.nlil[f] = base;
}

namespace {

template <bool LIL>
int pose_launch(pslfe_ctx* ctx, int nframes, const PslPose* d_Tin, const PslPoseEdge* d_edges, const int32_t* d_nedges, int estride,
                const PslCamera* cam, PslPose* d_Tout, uint8_t* d_outlier, int32_t* d_ngood, PslPoseInfo* d_info,
                const PoseLilArgs& B = PoseLilArgs{nullptr, nullptr, 0, nullptr}) {
    PoseArgs A;
    A.Tin = d_Tin; A.edges = d_edges; A.nedges = d_nedges; A.estride = estride;
    A.lds_edges = estride < PSL_POSE_LDS_EDGES ? estride : PSL_POSE_LDS_EDGES;
    A.K.fx = (double)cam->fx; A.K.fy = (double)cam->fy; A.K.cx = (double)cam->cx; A.K.cy = (double)cam->cy; A.K.bf = (double)cam->bf;
    A.Tout = d_Tout; A.outlier = d_outlier; A.ngood = d_ngood; A.info = d_info;
    const size_t lds = (size_t)A.lds_edges * sizeof(PslPoseEdge);
    {
        PSL_STAGE_BEGIN(ctx, "pose.optimize");
        k_pose_optimize<LIL><<<nframes, PSL_POSE_BS, lds, ctx->stream>>>(A, B);
        PSL_STAGE_END(ctx, "pose.optimize");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

// the host form of one frame: upload, launch k_pose_optimize<LIL>, download.  who: the entry point, which has checked its arguments;
// without LIL the LIL arguments are not used.
template <bool LIL>
int pose_host_form(pslfe_ctx* ctx, const char* who, const PslPose* Tcw, const PslPoseEdge* edges, int nedges, const PslPoseLilEdge* lil,
                   int nlil, const PslCamera* cam, PslPose* Tcw_out, uint8_t* outlier, uint8_t* outlier_lil, int* ngood) {
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int32_t n32 = nedges, m32 = nlil;
    PoseLilArgs B = {nullptr, nullptr, 0, nullptr};
    PslPose* d_T = psl_scratch_up(ctx, Tcw, 1, st, &e);
    const PslPoseEdge* d_edges = psl_scratch_up(ctx, nedges ? edges : nullptr, (size_t)nedges, st, &e);
    if constexpr (LIL) B.lil = psl_scratch_up(ctx, nlil ? lil : nullptr, (size_t)nlil, st, &e);
    const int32_t* d_n = psl_scratch_up(ctx, &n32, 1, st, &e);
    if constexpr (LIL) B.nlil = psl_scratch_up(ctx, &m32, 1, st, &e);
    uint8_t* d_out = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)nedges, st, &e);   // outputs: not read, not written below 3 edges
    if constexpr (LIL) B.outlier = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)nlil, st, &e);
    int32_t* d_ng = psl_scratch_up(ctx, (const int32_t*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    B.lstride = nlil;
    if (int rc = pose_launch<LIL>(ctx, 1, d_T, d_edges, d_n, nedges, cam, d_T, d_out, d_ng, nullptr, B)) return rc;
    int32_t ng = 0;
    PSL_HIP(hipMemcpyAsync(Tcw_out, d_T, sizeof(PslPose), hipMemcpyDeviceToHost, st));
    if (nedges + nlil >= 3) {
        if (nedges) PSL_HIP(hipMemcpyAsync(outlier, d_out, (size_t)nedges, hipMemcpyDeviceToHost, st));
        if (nlil) PSL_HIP(hipMemcpyAsync(outlier_lil, B.outlier, (size_t)nlil, hipMemcpyDeviceToHost, st));
    }
    PSL_HIP(hipMemcpyAsync(&ng, d_ng, sizeof(ng), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *ngood = ng;
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_pose_optimize_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw_in, const PslPoseEdge* d_edges, const int32_t* d_nedges,
                               int estride, const PslCamera* cam, PslPose* d_Tcw_out, uint8_t* d_outlier, int32_t* d_ngood,
                               PslPoseInfo* d_info) {
    static const char* who = "pslfe_pose_optimize_device";
    PSL_REQUIRE(nframes >= 0 && estride >= 0, PSLFE_E_INVALID, "%s: nframes = %d, estride = %d", who, nframes, estride);
    if (nframes == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && cam, PSLFE_E_INVALID, "%s: NULL context or camera", who);
    PSL_REQUIRE(d_Tcw_in && d_nedges && d_Tcw_out && d_ngood, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(estride == 0 || (d_edges && d_outlier), PSLFE_E_INVALID, "%s: NULL edges or outlier bytes with estride = %d", who, estride);
    PSL_HIP(hipSetDevice(ctx->device));
    return pose_launch<false>(ctx, nframes, d_Tcw_in, d_edges, d_nedges, estride, cam, d_Tcw_out, d_outlier, d_ngood, d_info);
}

int pslfe_pose_optimize(pslfe_ctx* ctx, const PslPose* Tcw, const PslPoseEdge* edges, int nedges, const PslCamera* cam, PslPose* Tcw_out,
                        uint8_t* outlier, int* ngood) {
    static const char* who = "pslfe_pose_optimize";
    PSL_REQUIRE(nedges >= 0, PSLFE_E_INVALID, "%s: nedges = %d", who, nedges);
    PSL_REQUIRE(ctx && cam && Tcw && Tcw_out && ngood, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(nedges == 0 || (edges && outlier), PSLFE_E_INVALID, "%s: NULL edges or outlier bytes with nedges = %d", who, nedges);
    return pose_host_form<false>(ctx, who, Tcw, edges, nedges, nullptr, 0, cam, Tcw_out, outlier, nullptr, ngood);
}

int pslfe_pose_optimize_lil_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw_in, const PslPoseEdge* d_edges, const int32_t* d_nedges,
                                   int estride, const PslPoseLilEdge* d_lil, const int32_t* d_nlil, int lstride, const PslCamera* cam,
                                   PslPose* d_Tcw_out, uint8_t* d_outlier, uint8_t* d_outlier_lil, int32_t* d_ngood, PslPoseInfo* d_info) {
    static const char* who = "pslfe_pose_optimize_lil_device";
    PSL_REQUIRE(nframes >= 0 && estride >= 0 && lstride >= 0, PSLFE_E_INVALID, "%s: nframes = %d, estride = %d, lstride = %d", who, nframes,
                estride, lstride);
    if (nframes == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && cam, PSLFE_E_INVALID, "%s: NULL context or camera", who);
    PSL_REQUIRE(d_Tcw_in && d_nedges && d_nlil && d_Tcw_out && d_ngood, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(estride == 0 || (d_edges && d_outlier), PSLFE_E_INVALID, "%s: NULL edges or outlier bytes with estride = %d", who, estride);
    PSL_REQUIRE(lstride == 0 || (d_lil && d_outlier_lil), PSLFE_E_INVALID, "%s: NULL LIL edges or outlier bytes with lstride = %d", who, lstride);
    PSL_HIP(hipSetDevice(ctx->device));
    const PoseLilArgs B = {d_lil, d_nlil, lstride, d_outlier_lil};
    return pose_launch<true>(ctx, nframes, d_Tcw_in, d_edges, d_nedges, estride, cam, d_Tcw_out, d_outlier, d_ngood, d_info, B);
}

int pslfe_pose_optimize_lil(pslfe_ctx* ctx, const PslPose* Tcw, const PslPoseEdge* edges, int nedges, const PslPoseLilEdge* lil, int nlil,
                            const PslCamera* cam, PslPose* Tcw_out, uint8_t* outlier, uint8_t* outlier_lil, int* ngood) {
    static const char* who = "pslfe_pose_optimize_lil";
    PSL_REQUIRE(nedges >= 0 && nlil >= 0, PSLFE_E_INVALID, "%s: nedges = %d, nlil = %d", who, nedges, nlil);
    PSL_REQUIRE(ctx && cam && Tcw && Tcw_out && ngood, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(nedges == 0 || (edges && outlier), PSLFE_E_INVALID, "%s: NULL edges or outlier bytes with nedges = %d", who, nedges);
    PSL_REQUIRE(nlil == 0 || (lil && outlier_lil), PSLFE_E_INVALID, "%s: NULL LIL edges or outlier bytes with nlil = %d", who, nlil);
    return pose_host_form<true>(ctx, who, Tcw, edges, nedges, lil, nlil, cam, Tcw_out, outlier, outlier_lil, ngood);
}

int pslfe_pose_lil_edges_device(pslfe_ctx* ctx, int nframes, const double* d_le_l, int le_stride, const double* d_cross2d, int plane_stride,
                                const int32_t* d_nplanes, const int32_t* d_lil_index, const PslMapLil* d_map, int nmap, PslPoseLilEdge* d_lil,
                                int32_t* d_edge_plane, int32_t* d_nlil, int lstride) {
    static const char* who = "pslfe_pose_lil_edges_device";
    PSL_REQUIRE(nframes >= 0 && le_stride >= 0 && plane_stride >= 0 && nmap >= 0 && lstride >= 0, PSLFE_E_INVALID,
                "%s: nframes = %d, le_stride = %d, plane_stride = %d, nmap = %d, lstride = %d", who, nframes, le_stride, plane_stride, nmap, lstride);
    if (nframes == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && d_nplanes && d_nlil, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(plane_stride == 0 || (d_cross2d && d_lil_index), PSLFE_E_INVALID, "%s: NULL planes with plane_stride = %d", who, plane_stride);
    PSL_REQUIRE(le_stride == 0 || d_le_l, PSLFE_E_INVALID, "%s: NULL mvle_l rows with le_stride = %d", who, le_stride);
    PSL_REQUIRE(nmap == 0 || d_map, PSLFE_E_INVALID, "%s: NULL map LILs with nmap = %d", who, nmap);
    PSL_REQUIRE(lstride == 0 || d_lil, PSLFE_E_INVALID, "%s: NULL edges with lstride = %d", who, lstride);
    PSL_HIP(hipSetDevice(ctx->device));
    PoseLilEdgeArgs A;
    A.le_l = d_le_l; A.cross2d = d_cross2d; A.nplanes = d_nplanes; A.lil_index = d_lil_index; A.map = d_map;
    A.le_stride = le_stride; A.plane_stride = plane_stride; A.nmap = nmap;
    A.lil = d_lil; A.edge_plane = d_edge_plane; A.nlil = d_nlil; A.lstride = lstride;
    {
        PSL_STAGE_BEGIN(ctx, "pose.lil_edges");
        k_pose_lil_edges<<<nframes, 256, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "pose.lil_edges");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int pslfe_pose_edges_from_matches_device(pslfe_frame* frame, int slot0, int nframes, const int32_t* d_mp_index, const PslMapPointGeom* d_mp,
                                         int mpstride, const float* inv_level_sigma2, int nlevels, PslPoseEdge* d_edges, int32_t* d_edge_kp,
                                         int32_t* d_nedges, int estride) {
    static const char* who = "pslfe_pose_edges_from_matches_device";
    PSL_REQUIRE(nframes >= 0 && estride >= 0 && mpstride >= 0, PSLFE_E_INVALID, "%s: nframes = %d, estride = %d, mpstride = %d", who, nframes,
                estride, mpstride);
    if (nframes == 0) return PSLFE_OK;
    PSL_REQUIRE(frame, PSLFE_E_INVALID, "%s: NULL frame store", who);
    PSL_REQUIRE(slot0 >= 0 && slot0 + nframes <= frame->max_frames, PSLFE_E_INVALID, "%s: slots %d..%d of %d", who, slot0, slot0 + nframes - 1,
                frame->max_frames);
    for (int s = slot0; s < slot0 + nframes; ++s) PSL_REQUIRE(frame->slot_set[s], PSLFE_E_STATE, "%s: slot %d not set", who, s);
    PSL_REQUIRE(nlevels >= 1 && nlevels <= PSLFE_MAX_LEVELS && inv_level_sigma2, PSLFE_E_INVALID, "%s: nlevels = %d (1..%d) or NULL table", who,
                nlevels, PSLFE_MAX_LEVELS);
    PSL_REQUIRE(d_mp_index && d_nedges, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(mpstride == 0 || d_mp, PSLFE_E_INVALID, "%s: NULL map points with mpstride = %d", who, mpstride);
    PSL_REQUIRE(estride == 0 || d_edges, PSLFE_E_INVALID, "%s: NULL edges with estride = %d", who, estride);
    pslfe_ctx* ctx = frame->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    PoseEdgeArgs A;
    A.S = frame->S; A.slot0 = slot0; A.mp_index = d_mp_index; A.mp = d_mp; A.mpstride = mpstride; A.nlevels = nlevels;
    for (int l = 0; l < PSLFE_MAX_LEVELS; ++l) A.inv_sigma2[l] = l < nlevels ? inv_level_sigma2[l] : 0.f;
    A.edges = d_edges; A.edge_kp = d_edge_kp; A.nedges = d_nedges; A.estride = estride;
    {
        PSL_STAGE_BEGIN(ctx, "pose.edges");
        k_pose_edges<<<nframes, 256, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "pose.edges");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int pslfe_pose_mp_index_from_matches_device(pslfe_frame* frame, int nframes, const int32_t* d_match, const int32_t* d_owner, const int32_t* d_nq,
                                            int qstride, int32_t* d_mp_index) {
    static const char* who = "pslfe_pose_mp_index_from_matches_device";
    PSL_REQUIRE(nframes >= 0 && qstride >= 0, PSLFE_E_INVALID, "%s: nframes = %d, qstride = %d", who, nframes, qstride);
    if (nframes == 0) return PSLFE_OK;
    PSL_REQUIRE(frame && d_nq && d_mp_index, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(qstride == 0 || (d_match && d_owner), PSLFE_E_INVALID, "%s: NULL rows with qstride = %d", who, qstride);
    pslfe_ctx* ctx = frame->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    {
        PSL_STAGE_BEGIN(ctx, "pose.mp_index");
        k_pose_mp_index<<<nframes, 256, 0, ctx->stream>>>(d_match, d_owner, d_nq, qstride, frame->cap, d_mp_index);
        PSL_STAGE_END(ctx, "pose.mp_index");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // extern "C"
