// libpslfe: PnPsolver (src/PnPsolver.cc), the EPnP RANSAC of Tracking::Relocalization (src/Tracking.cc:2075-2101), for K candidate
// keyframes in one launch, with its set-up (the constructor's loop) and the masking of the matches by the inliers (:2119-2128).
// Product code.
// Who owns what.  pnp_solver_kernels.h holds everything a single thread computes - the staging of a row, EPnP in stages, the
// inlier test of a row - and the reference's loop on one core (psl_pnp_iterate), which tools/dropin/pnp_main.cpp runs and
// tests/pnp_cases.py restates in numpy; glibc's rand() and the draw are those of ransac_kernels.h, shared with the other RANSAC
// solvers, and its reading of OpenCV's Jacobi SVD is written out on the workspace's offsets (psl_pnp_jacobi).  Here: which thread
// computes which hypothesis, which sum and which row, the LDS copy of the staged rows, the error paths, and the driver in blocks.
//
// The driver in blocks.  PnPsolver::iterate draws four rows, solves, counts, and - when the count reaches mRansacMinInliers - keeps the
// hypothesis as the best on > and refines on the best inlier set; it returns at the first Refine that succeeds.  The draws never depend
// on a result, so the kernel draws and solves a block of up to 16 iterations at once and counts their inliers; then it walks the block
// in iteration order and does for every hypothesis with count >= min what the reference does: update the best on >, Refine, stop at
// the first success (the later hypotheses of the block are discarded, mnIterations is the number of the one that won).  A block never
// runs past the call's iterations, max(mRansacMaxIts - mnIterations, n_iterations): the reference's loop condition is an ||.
//
// Layout.  One workgroup of 256 threads per candidate, resident through all blocks.  Rows: the first PSL_PNP_LDS_ROWS staged rows (u, v,
// X, Y, Z, sigma2 * th2) lie in LDS with a stride of 7 words (odd: 32 consecutive rows, 32 banks); a row beyond them is staged from
// HBM where it is used, with the same arithmetic.  Hypotheses: lane = hypothesis.  A four-point compute_pose is about 15 kflop of
// dependent f64 on 372 doubles of workspace (the 12x12 M^T M / Ut alone is 1152 bytes), far more than a lane's registers, so the
// workspaces lie in LDS, interleaved (element k of hypothesis h at double k * 16 + h), and a block is 16 hypotheses: 46.5 KB, which
// with the rows stays under the 64 KB a workgroup gets without an opt-in.  Hypothesis h is computed by thread 16 h, four per wave, so
// a block occupies all four SIMDs; f64 FMA-class operations issue at a quarter rate per lane anyway and the chain is latency-bound, so
// more lanes per wave would only queue on the same SIMD.  The alternative, a group of lanes per hypothesis, would parallelise the 78
// sums of M^T M and the row pairs of a Jacobi sweep but needs a cross-lane exchange per rotation; it was not chosen for the first
// version.  Counting: wave w counts hypotheses w, w + 4, ... over the rows, 64 at a time, by ballot and popcount.
// Refine is cooperative: every sum over the inlier rows (3 + 6 + 78 + 6 + 9 + 1 per trial) is one thread's sequential sum in row
// order - parallel across entries, never a tree across rows - so its bits are those of the host loop; the SVDs between them run on
// thread 0.  The best inlier set lives in the caller's d_best_flags (HBM), written by all threads and read back after a barrier.
#include <string.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "pslfe_internal.h"
#include "match_kernels.h"
#include "proj_kernels.h"
#include "pnp_solver_kernels.h"

#define PSL_PNP_BS 256
#define PSL_PNP_B 16
#define PSL_PNP_LDS_ROWS 384

static_assert(sizeof(PslPnpRow) == 6 * sizeof(float), "a row is 6 floats");

struct PnpSolveArgs {
    const PslPnpRow* rows;
    const int32_t* nrows;
    int rstride, lds_rows;
    PslPnpCam K;
    float th2;
    const int32_t* tab;            // [rstride + 1][2]: mRansacMaxIts, mRansacMinInliers by row count
    int n_iterations;
    uint32_t seed0;
    const PslPnpResult* state;
    uint8_t* best_flags;
    PslPnpResult* res;
    uint8_t* inliers;
};

extern __shared__ float s_pnp_rows[];

__device__ __forceinline__ void pnp_write_result(PslPnpResult* r, int status, int iterations, int inliers, int best, int min_inliers, const float* T,
                                                 const float* bestT) {
    PslPnpResult o;
    o.status = status; o.iterations = iterations; o.inliers = inliers; o.best_inliers = best; o.min_inliers = min_inliers;
    for (int i = 0; i < 9; ++i) { o.Tcw.R[i] = T ? T[i] : 0.f; o.best_Tcw.R[i] = bestT ? bestT[i] : 0.f; }
    for (int i = 0; i < 3; ++i) { o.Tcw.t[i] = T ? T[9 + i] : 0.f; o.best_Tcw.t[i] = bestT ? bestT[9 + i] : 0.f; }
    *r = o;
}

// the inliers of the rows under pose Rt, counted by the whole workgroup; flags (may be NULL) gets the byte of every row
__device__ __forceinline__ int pnp_count_all(const PslPnpRows& R, int n, const double* Rt, const PslPnpCam& K, uint8_t* flags, int* s_part) {
    const int tid = threadIdx.x;
    int cnt = 0;
    for (int i0 = 0; i0 < n; i0 += PSL_PNP_BS) {   // uniform
        const int i = i0 + tid;
        int in = 0;
        if (i < n) {
            float q[6];
            psl_pnp_load(&R, i, q);
            in = psl_pnp_inlier(q, Rt, &K);
            if (flags) flags[i] = (uint8_t)in;
        }
        cnt += __popcll(__ballot(in));
    }
    __syncthreads();
    if ((tid & 63) == 0) s_part[tid >> 6] = cnt;
    __syncthreads();
    return s_part[0] + s_part[1] + s_part[2] + s_part[3];
}

// compute_pose on the rows whose flag is set, by the workgroup: ws is workspace 0 of the block (stride PSL_PNP_B); R, t are left in RTB
__device__ void pnp_refine_pose(double* ws, const PslPnpRows& R, const PslPnpSel& S, const PslPnpCam& K) {
    constexpr int ES = PSL_PNP_B;
    const int tid = threadIdx.x;
    const double dn = (double)S.n;
#define W_(k) ws[(size_t)(k) * ES]
    if (tid < 3) W_(PSL_PNP_CWS + tid) = PSL_PO_DIV(psl_pnp_sum_cw0<ES>(&R, &S, tid), dn);
    __syncthreads();
    if (tid < 6) {
        int a, b;
        psl_pnp_tri3(tid, &a, &b);
        const double v = psl_pnp_sum_pwpw<ES>(ws, &R, &S, tid);
        W_(PSL_PNP_M3 + 3 * a + b) = v; W_(PSL_PNP_M3 + 3 * b + a) = v;
    }
    __syncthreads();
    if (tid == 0) psl_pnp_control_points<ES>(ws, S.n);
    __syncthreads();
    if (tid < 78) {
        int p, q;
        psl_pnp_tri12(tid, &p, &q);
        const double v = psl_pnp_sum_mtm<ES>(ws, &R, &S, &K, p, q);
        W_(PSL_PNP_AT + 12 * p + q) = v; W_(PSL_PNP_AT + 12 * q + p) = v;
    }
    __syncthreads();
    if (tid == 0) psl_pnp_null_space<ES>(ws);
    for (int which = 1; which <= 3; ++which) {   // uniform
        if (tid == 0) {
            psl_pnp_betas_approx<ES>(ws, which);
            psl_pnp_gauss_newton<ES>(ws);
            psl_pnp_ccs<ES>(ws);
            psl_pnp_sign<ES>(ws, &R, &S);
        }
        __syncthreads();
        if (tid < 6) {
            const double v = PSL_PO_DIV(psl_pnp_sum_c0<ES>(ws, &R, &S, tid), dn);
            W_(PSL_PNP_PC0 + tid) = v;
        }
        __syncthreads();
        if (tid < 9) {
            const double v = psl_pnp_sum_abt<ES>(ws, &R, &S, tid);
            W_(PSL_PNP_M3 + tid) = v;
        }
        __syncthreads();
        if (tid == 0) {
            psl_pnp_rt<ES>(ws);
            W_(PSL_PNP_ERR) = PSL_PO_DIV(psl_pnp_sum_reproj<ES>(ws, &R, &S, &K), dn);
            psl_pnp_keep<ES>(ws, which);
        }
        __syncthreads();
    }
#undef W_
}

__global__ __launch_bounds__(PSL_PNP_BS) void k_pnp_solve(PnpSolveArgs A) {
    __shared__ double s_ws[PSL_PNP_WS * PSL_PNP_B];
    __shared__ double s_pose[PSL_PNP_B][12];
    __shared__ int s_idx[PSL_PNP_B][4];
    __shared__ int s_cnt[PSL_PNP_B];
    __shared__ int s_part[4];
    __shared__ float s_bestT[12];
    __shared__ PslRsRand s_rand;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.nrows[c];
    PslPnpResult* res = A.res + c;
    int start_it = 0, best_in = 0;
    if (A.state) { start_it = A.state[c].iterations; best_in = A.state[c].best_inliers; }
    if (tid < 12) s_bestT[tid] = A.state ? (tid < 9 ? A.state[c].best_Tcw.R[tid] : A.state[c].best_Tcw.t[tid - 9]) : 0.f;
    __syncthreads();   // every thread has read the state before any result is written: d_res may be d_state_in
    if (n < 0 || n > A.rstride || start_it < 0 || best_in < 0) {   // uniform: an error code the set-up left there, a count the rows
        // cannot hold, or a negative state; the status alone is written (the other fields 0) and no flag byte
        if (tid == 0) pnp_write_result(res, n > A.rstride ? PSLFE_E_CAPACITY : PSLFE_E_INVALID, 0, 0, 0, 0, nullptr, nullptr);
        return;
    }
    const int max_its = A.tab[2 * n], min_inliers = A.tab[2 * n + 1];
    uint8_t* flags = A.inliers + (size_t)c * A.rstride;
    uint8_t* bflags = A.best_flags + (size_t)c * A.rstride;
    if (n < min_inliers) {   // N < mRansacMinInliers: bNoMore at once (:173-177)
        for (int i = tid; i < n; i += PSL_PNP_BS) flags[i] = 0;
        if (tid == 0) pnp_write_result(res, 2, start_it, 0, best_in, min_inliers, nullptr, s_bestT);
        return;
    }
    const float* rows = reinterpret_cast<const float*>(A.rows + (size_t)c * A.rstride);
    const int lds_n = n < A.lds_rows ? n : A.lds_rows;
    for (int i = tid; i < lds_n; i += PSL_PNP_BS) {
        float q[6];
        psl_pnp_stage(rows + 6 * (size_t)i, A.th2, q);
#pragma unroll
        for (int k = 0; k < 6; ++k) s_pnp_rows[PSL_PNP_ROW_FLOATS * i + k] = q[k];
    }
    const PslPnpRows R = {s_pnp_rows, lds_n, rows, A.th2};
    int it = start_it, best = best_in;
    int left = max_its - start_it;
    if (left < A.n_iterations) left = A.n_iterations;
    if (tid == 0 && left > 0) {   // a call that runs no iteration draws nothing
        psl_rs_srand(&s_rand, A.seed0 + (uint32_t)c);
        for (int i = 0; i < 4 * start_it; ++i) psl_rs_rand(&s_rand);
    }
    __syncthreads();
    for (;;) {   // uniform
        const int nb = left < PSL_PNP_B ? left : PSL_PNP_B;
        if (nb <= 0) break;
        if (tid == 0)
            for (int h = 0; h < nb; ++h) psl_rs_draw<4>(&s_rand, n, s_idx[h]);
        __syncthreads();
        if ((tid & 15) == 0 && (tid >> 4) < nb) {
            const int h = tid >> 4;
            const PslPnpSel S = {s_idx[h], nullptr, 4, 4};
            psl_pnp_compute_pose<PSL_PNP_B>(s_ws + h, &R, &S, &A.K);
            for (int k = 0; k < 12; ++k) s_pose[h][k] = s_ws[(size_t)(PSL_PNP_RTB + k) * PSL_PNP_B + h];
        }
        __syncthreads();
        for (int h = wave; h < nb; h += PSL_PNP_BS / 64) {   // uniform in the wave
            double Rt[12];
#pragma unroll
            for (int k = 0; k < 12; ++k) Rt[k] = s_pose[h][k];
            int cnt = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                int in = 0;
                if (i < n) {
                    float q[6];
                    psl_pnp_load(&R, i, q);
                    in = psl_pnp_inlier(q, Rt, &A.K);
                }
                cnt += __popcll(__ballot(in));
            }
            if (lane == 0) s_cnt[h] = cnt;
        }
        __syncthreads();
        for (int h = 0; h < nb; ++h) {   // the reference's order (:209-238); every branch is uniform
            const int cnt = s_cnt[h];
            if (cnt < min_inliers) continue;
            double Rt[12];
            if (cnt > best) {   // mvbBestInliers, mnBestInliers, mBestTcw
#pragma unroll
                for (int k = 0; k < 12; ++k) Rt[k] = s_pose[h][k];
                for (int i = tid; i < n; i += PSL_PNP_BS) {
                    float q[6];
                    psl_pnp_load(&R, i, q);
                    bflags[i] = (uint8_t)psl_pnp_inlier(q, Rt, &A.K);
                }
                best = cnt;
                if (tid < 12) s_bestT[tid] = (float)Rt[tid];
                __threadfence_block();
                __syncthreads();
            }
            // Refine (:260-305) on mvbBestInliers
            int nbest = 0;
            for (int i0 = 0; i0 < n; i0 += PSL_PNP_BS) {
                const int i = i0 + tid;
                nbest += __popcll(__ballot(i < n && bflags[i] != 0));
            }
            if (lane == 0) s_part[wave] = nbest;
            __syncthreads();
            nbest = s_part[0] + s_part[1] + s_part[2] + s_part[3];
            __syncthreads();
            const PslPnpSel SR = {nullptr, bflags, n, nbest};
            pnp_refine_pose(s_ws, R, SR, A.K);
#pragma unroll
            for (int k = 0; k < 12; ++k) Rt[k] = s_ws[(size_t)(PSL_PNP_RTB + k) * PSL_PNP_B];
            const int rc = pnp_count_all(R, n, Rt, A.K, nullptr, s_part);
            if (rc > min_inliers) {   // mRefinedTcw, mvbRefinedInliers
                pnp_count_all(R, n, Rt, A.K, flags, s_part);
                if (tid == 0) {
                    float T[12];
                    psl_pnp_to_float(Rt, T);
                    pnp_write_result(res, 1, it + h + 1, rc, best, min_inliers, T, s_bestT);
                }
                return;
            }
            __syncthreads();
        }
        it += nb;
        left -= nb;
    }
    // after the loop (:241-257)
    const bool no_more = it >= max_its, have = no_more && best >= min_inliers;
    for (int i = tid; i < n; i += PSL_PNP_BS) flags[i] = have ? bflags[i] : (uint8_t)0;
    if (tid == 0) pnp_write_result(res, (no_more ? 2 : 0) | (have ? 1 : 0), it, have ? best : 0, best, min_inliers, have ? s_bestT : nullptr, s_bestT);
}

// ---- the rows of a candidate from its matches: the constructor's loop (:78-101) -------------------------------------------------------
struct PnpRowsArgs {
    FrameStore S;
    int slot;
    const int32_t* mp_index;   // [ncand][S.cap]
    const PslMapPointGeom* mp;
    int mpstride;
    float sigma2[PSLFE_MAX_LEVELS];
    int nlevels;
    PslPnpRow* rows;
    int32_t* row_kp;
    int32_t* nrows;
    int rstride;
};

// one workgroup per candidate: the keypoints in chunks of 256, compacted in keypoint order (psl_wg_compact of proj_kernels.h)
__global__ __launch_bounds__(256) void k_pnp_rows(PnpRowsArgs A) {
    __shared__ int s_cnt[4];
    const int c = blockIdx.x, tid = threadIdx.x;
    const int n = min(A.S.meta[A.slot].n, A.S.cap);
    const PslKeyPoint* kps = A.S.kps + (size_t)A.slot * A.S.cap;
    const int32_t* idx = A.mp_index + (size_t)c * A.S.cap;
    const PslMapPointGeom* mp = A.mp + (size_t)c * A.mpstride;
    PslPnpRow* rows = A.rows + (size_t)c * A.rstride;
    int32_t* row_kp = A.row_kp ? A.row_kp + (size_t)c * A.rstride : nullptr;
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
        if (m >= 0 && pos < A.rstride) {
            const PslKeyPoint kp = kps[i];
            const int oct = min(max(kp.octave, 0), A.nlevels - 1);
            PslPnpRow r;
            r.u = kp.x; r.v = kp.y; r.X = mp[m].x; r.Y = mp[m].y; r.Z = mp[m].z; r.sigma2 = A.sigma2[oct];
            rows[pos] = r;
            if (row_kp) row_kp[pos] = i;
        }
    }
    if (tid == 0) A.nrows[c] = base;
}

// ---- the matches that are inliers (src/Tracking.cc:2119-2128): one workgroup per candidate --------------------------------------------
__global__ __launch_bounds__(256) void k_pnp_mask(const int32_t* __restrict__ mp_index, const int32_t* __restrict__ row_kp,
                                                  const uint8_t* __restrict__ inliers, const int32_t* __restrict__ nrows, int rstride, int kpstride,
                                                  int32_t* __restrict__ out) {
    const int c = blockIdx.x, tid = threadIdx.x;
    const int32_t* in = mp_index + (size_t)c * kpstride;
    int32_t* o = out + (size_t)c * kpstride;
    const int n = min(max(nrows[c], 0), rstride);
    for (int i = tid; i < kpstride; i += 256) o[i] = -1;
    __syncthreads();
    for (int r = tid; r < n; r += 256) {
        if (!inliers[(size_t)c * rstride + r]) continue;
        const int kp = row_kp[(size_t)c * rstride + r];
        if (kp >= 0 && kp < kpstride) o[kp] = in[kp];
    }
}

namespace {

int pnp_solve_check(const char* who, int ncand, int rstride, double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2,
                    int n_iterations) {
    PSL_REQUIRE(ncand >= 0 && rstride >= 0, PSLFE_E_INVALID, "%s: ncand = %d, rstride = %d", who, ncand, rstride);
    PSL_REQUIRE(min_inliers >= 0 && max_its >= 1 && n_iterations >= 0, PSLFE_E_INVALID, "%s: min_inliers = %d, max_its = %d, n_iterations = %d", who,
                min_inliers, max_its, n_iterations);
    PSL_REQUIRE(min_set == PSL_PNP_MIN_SET, PSLFE_E_INVALID, "%s: min_set = %d; the solver is EPnP on 4 points", who, min_set);
    PSL_REQUIRE(prob > 0.0 && prob < 1.0, PSLFE_E_INVALID, "%s: prob = %g outside (0, 1)", who, prob);
    PSL_REQUIRE(epsilon == epsilon && th2 == th2, PSLFE_E_INVALID, "%s: NaN epsilon or th2", who);
    return PSLFE_OK;
}

// mRansacMaxIts and mRansacMinInliers of the row counts 0 .. rstride.  Tables are kept for the life of the library, one per set of
// parameters (a process uses one or two), so a reference handed out stays valid and an upload may read it after the call has returned.
const std::vector<int32_t>& pnp_budget_table(double prob, int min_inliers, int max_its, float epsilon, int rstride) {
    static std::mutex mu;
    static std::map<std::tuple<double, int, int, float, int>, std::vector<int32_t>> tables;
    std::lock_guard<std::mutex> lock(mu);
    std::vector<int32_t>& t = tables[std::make_tuple(prob, min_inliers, max_its, epsilon, rstride)];
    if (t.empty()) {
        t.assign(2 * ((size_t)rstride + 1), 1);
        for (int N = 0; N <= rstride; ++N) {
            int mn = 0;
            t[2 * (size_t)N] = psl_pnp_max_iterations(prob, min_inliers, max_its, PSL_PNP_MIN_SET, epsilon, N, &mn);
            t[2 * (size_t)N + 1] = mn;
        }
    }
    return t;
}

// the caller has called psl_scratch_begin when `own_scratch` is 0
int pnp_solve_launch(pslfe_ctx* ctx, const char* who, int ncand, const PslPnpRow* d_rows, const int32_t* d_nrows, int rstride, const PslCamera* cam,
                     double prob, int min_inliers, int max_its, float epsilon, float th2, uint32_t seed0, const PslPnpResult* d_state_in,
                     uint8_t* d_best_flags, int n_iterations, PslPnpResult* d_res, uint8_t* d_inliers, int own_scratch) {
    PnpSolveArgs A;
    A.rows = d_rows; A.nrows = d_nrows; A.rstride = rstride;
    A.lds_rows = rstride < PSL_PNP_LDS_ROWS ? rstride : PSL_PNP_LDS_ROWS;
    A.K.fu = (double)cam->fx; A.K.fv = (double)cam->fy; A.K.uc = (double)cam->cx; A.K.vc = (double)cam->cy;
    A.th2 = th2; A.n_iterations = n_iterations; A.seed0 = seed0;
    A.state = d_state_in; A.best_flags = d_best_flags; A.res = d_res; A.inliers = d_inliers;
    const std::vector<int32_t>& tab = pnp_budget_table(prob, min_inliers, max_its, epsilon, rstride);
    if (own_scratch)
        if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    A.tab = psl_scratch_up(ctx, tab.data(), tab.size(), ctx->stream, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    const size_t lds = (size_t)A.lds_rows * PSL_PNP_ROW_FLOATS * sizeof(float);
    {
        PSL_STAGE_BEGIN(ctx, "pnp.solve");
        k_pnp_solve<<<ncand, PSL_PNP_BS, lds, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "pnp.solve");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_pnp_rows_from_matches_device(pslfe_frame* frame, int slot, int ncand, const int32_t* d_mp_index, const PslMapPointGeom* d_mp,
                                       int mpstride, const float* level_sigma2, int nlevels, PslPnpRow* d_rows, int32_t* d_row_kp,
                                       int32_t* d_nrows, int rstride) {
    static const char* who = "pslfe_pnp_rows_from_matches_device";
    PSL_REQUIRE(ncand >= 0 && rstride >= 0 && mpstride >= 0, PSLFE_E_INVALID, "%s: ncand = %d, rstride = %d, mpstride = %d", who, ncand, rstride,
                mpstride);
    if (ncand == 0) return PSLFE_OK;
    PSL_REQUIRE(frame, PSLFE_E_INVALID, "%s: NULL frame store", who);
    PSL_REQUIRE(slot >= 0 && slot < frame->max_frames, PSLFE_E_INVALID, "%s: slot %d of %d", who, slot, frame->max_frames);
    PSL_REQUIRE(frame->slot_set[slot], PSLFE_E_STATE, "%s: slot %d not set", who, slot);
    PSL_REQUIRE(nlevels >= 1 && nlevels <= PSLFE_MAX_LEVELS && level_sigma2, PSLFE_E_INVALID, "%s: nlevels = %d (1..%d) or NULL table", who, nlevels,
                PSLFE_MAX_LEVELS);
    PSL_REQUIRE(d_mp_index && d_nrows, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(mpstride == 0 || d_mp, PSLFE_E_INVALID, "%s: NULL map points with mpstride = %d", who, mpstride);
    PSL_REQUIRE(rstride == 0 || d_rows, PSLFE_E_INVALID, "%s: NULL rows with rstride = %d", who, rstride);
    pslfe_ctx* ctx = frame->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    PnpRowsArgs A;
    A.S = frame->S; A.slot = slot; A.mp_index = d_mp_index; A.mp = d_mp; A.mpstride = mpstride; A.nlevels = nlevels;
    for (int l = 0; l < PSLFE_MAX_LEVELS; ++l) A.sigma2[l] = l < nlevels ? level_sigma2[l] : 0.f;
    A.rows = d_rows; A.row_kp = d_row_kp; A.nrows = d_nrows; A.rstride = rstride;
    {
        PSL_STAGE_BEGIN(ctx, "pnp.rows");
        k_pnp_rows<<<ncand, 256, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "pnp.rows");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int pslfe_pnp_ransac_parameters(double prob, int min_inliers, int max_its, int min_set, float epsilon, int N, int* max_its_out,
                                int* min_inliers_out) {
    static const char* who = "pslfe_pnp_ransac_parameters";
    if (int rc = pnp_solve_check(who, 1, N, prob, min_inliers, max_its, min_set, epsilon, 0.f, 0)) return rc;
    PSL_REQUIRE(max_its_out && min_inliers_out, PSLFE_E_INVALID, "%s: NULL output", who);
    *max_its_out = psl_pnp_max_iterations(prob, min_inliers, max_its, min_set, epsilon, N, min_inliers_out);
    return PSLFE_OK;
}

int pslfe_pnp_solve_device(pslfe_ctx* ctx, int ncand, const PslPnpRow* d_rows, const int32_t* d_nrows, int rstride, const PslCamera* cam,
                           double prob, int min_inliers, int max_its, int min_set, float epsilon, float th2, uint32_t seed0,
                           const PslPnpResult* d_state_in, uint8_t* d_best_flags, int n_iterations, PslPnpResult* d_res, uint8_t* d_inliers) {
    static const char* who = "pslfe_pnp_solve_device";
    if (int rc = pnp_solve_check(who, ncand, rstride, prob, min_inliers, max_its, min_set, epsilon, th2, n_iterations)) return rc;
    if (ncand == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && cam, PSLFE_E_INVALID, "%s: NULL context or camera", who);
    PSL_REQUIRE(d_nrows && d_res, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(rstride == 0 || (d_rows && d_best_flags && d_inliers), PSLFE_E_INVALID, "%s: NULL rows, best flags or inlier bytes with rstride = %d",
                who, rstride);
    PSL_HIP(hipSetDevice(ctx->device));
    return pnp_solve_launch(ctx, who, ncand, d_rows, d_nrows, rstride, cam, prob, min_inliers, max_its, epsilon, th2, seed0, d_state_in,
                            d_best_flags, n_iterations, d_res, d_inliers, 1);
}

int pslfe_pnp_solve(pslfe_ctx* ctx, const PslPnpRow* rows, int nrows, const PslCamera* cam, double prob, int min_inliers, int max_its,
                    int min_set, float epsilon, float th2, uint32_t seed, const PslPnpResult* state, uint8_t* best_flags, int n_iterations,
                    PslPnpResult* res, uint8_t* inliers) {
    static const char* who = "pslfe_pnp_solve";
    PSL_REQUIRE(nrows >= 0, PSLFE_E_INVALID, "%s: nrows = %d", who, nrows);
    PSL_REQUIRE(!state || (state->iterations >= 0 && state->best_inliers >= 0), PSLFE_E_INVALID, "%s: a negative state", who);
    if (int rc = pnp_solve_check(who, 1, nrows, prob, min_inliers, max_its, min_set, epsilon, th2, n_iterations)) return rc;
    PSL_REQUIRE(ctx && cam && res, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(nrows == 0 || (rows && best_flags && inliers), PSLFE_E_INVALID, "%s: NULL rows, best flags or inlier bytes with nrows = %d", who,
                nrows);
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int32_t n32 = nrows;
    PslPnpResult zero;
    memset(&zero, 0, sizeof(zero));
    const PslPnpRow* d_rows = psl_scratch_up(ctx, nrows ? rows : nullptr, (size_t)nrows, st, &e);
    const int32_t* d_n = psl_scratch_up(ctx, &n32, 1, st, &e);
    const PslPnpResult* d_state = psl_scratch_up(ctx, state ? state : &zero, 1, st, &e);
    uint8_t* d_best = psl_scratch_up(ctx, nrows ? (const uint8_t*)best_flags : nullptr, (size_t)nrows, st, &e);
    PslPnpResult* d_res = psl_scratch_up(ctx, (const PslPnpResult*)nullptr, 1, st, &e);
    uint8_t* d_inl = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)nrows, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    if (int rc = pnp_solve_launch(ctx, who, 1, d_rows, d_n, nrows, cam, prob, min_inliers, max_its, epsilon, th2, seed, d_state, d_best,
                                  n_iterations, d_res, d_inl, 0))
        return rc;
    PSL_HIP(hipMemcpyAsync(res, d_res, sizeof(PslPnpResult), hipMemcpyDeviceToHost, st));
    if (nrows) PSL_HIP(hipMemcpyAsync(inliers, d_inl, (size_t)nrows, hipMemcpyDeviceToHost, st));
    if (nrows) PSL_HIP(hipMemcpyAsync(best_flags, d_best, (size_t)nrows, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_pnp_mp_index_from_inliers_device(pslfe_ctx* ctx, int ncand, const int32_t* d_mp_index, const int32_t* d_row_kp, const uint8_t* d_inliers,
                                           const int32_t* d_nrows, int rstride, int kpstride, int32_t* d_mp_index_out) {
    static const char* who = "pslfe_pnp_mp_index_from_inliers_device";
    PSL_REQUIRE(ncand >= 0 && rstride >= 0 && kpstride >= 0, PSLFE_E_INVALID, "%s: ncand = %d, rstride = %d, kpstride = %d", who, ncand, rstride,
                kpstride);
    if (ncand == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && d_nrows, PSLFE_E_INVALID, "%s: NULL context or counts", who);
    PSL_REQUIRE(kpstride == 0 || (d_mp_index && d_mp_index_out && d_mp_index != d_mp_index_out), PSLFE_E_INVALID,
                "%s: NULL or aliased index arrays with kpstride = %d", who, kpstride);
    PSL_REQUIRE(rstride == 0 || (d_row_kp && d_inliers), PSLFE_E_INVALID, "%s: NULL row arrays with rstride = %d", who, rstride);
    PSL_HIP(hipSetDevice(ctx->device));
    {
        PSL_STAGE_BEGIN(ctx, "pnp.mask");
        k_pnp_mask<<<ncand, 256, 0, ctx->stream>>>(d_mp_index, d_row_kp, d_inliers, d_nrows, rstride, kpstride, d_mp_index_out);
        PSL_STAGE_END(ctx, "pnp.mask");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // extern "C"
