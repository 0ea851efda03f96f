// libpslfe: Sim3Solver (src/Sim3Solver.cc), the RANSAC of LoopClosing::ComputeSim3 (src/LoopClosing.cc:284-345), for K loop candidates
// in one launch.  Product code.
// Who owns what.  sim3_solver_kernels.h holds everything a single thread computes - the staging of a pair, Horn's closed form with
// OpenCV's eigen Jacobi (psl_ss_hypothesis), the inlier test of a pair - and the reference's loop on one core (psl_ss_iterate), which
// tools/dropin/sim3_solver_main.cpp runs and tests/sim3_solver_cases.py restates in numpy; glibc's rand() and the draw are those of
// ransac_kernels.h, shared with the other RANSAC solvers.  Here: which thread
// computes which hypothesis and which pair, the LDS copy of the staged pairs, the error paths, and the driver in blocks.
//
// The driver in blocks.  Sim3Solver::iterate evaluates one hypothesis after the other and returns at the first iteration i whose
// count c_i satisfies c_i >= mnBestInliers and c_i > mRansacMinInliers; mnBestInliers is the running maximum of best_in and the counts
// of the earlier iterations (an iteration with c_i >= best only raises best to c_i).  Hypothesis i depends on the draws alone, never on
// the counts, so the kernel may compute the hypotheses and counts of a block of up to 64 iterations at once and then walk the counts in
// iteration order with the running maximum: the first iteration that qualifies is the one the reference returns, mnIterations is its
// number, and the hypotheses after it in the block are discarded.  With best_in == 0 every earlier count was at most min_inliers, so
// the first count above min_inliers is also >= best; with best_in > 0 the walk applies the same rule with the maximum carried in.  A
// block never runs past the budget of the call (n_iterations) or of the solver (the tabulated mRansacMaxIts of the pair count).
//
// Layout.  One workgroup of 256 threads per candidate, resident through all blocks.  The staged pairs (12 floats: P1c, P2c, their two
// images, the two thresholds) of the first PSL_SS_LDS_PAIRS pairs are computed once into LDS with a row stride of 13 words, which is odd,
// so the 32 lanes of a ds_read_b32 group that read the same field of 32 consecutive pairs touch 32 different banks (a stride of 12
// would fold them onto 8); 1024 pairs take 52 KB.  A pair
// beyond that is staged from its HBM row where it is used, with the same arithmetic.  Thread 0 walks the candidate's rand() stream
// (ring in LDS) for the block's draws.  Hypothesis h of the block is computed by lane h % 16 of wave h / 16, so a full block occupies
// all four SIMDs of the CU and a round of 5 stays in one wave; Horn plus the 4x4 Jacobi is a few hundred dependent operations, independent
// across lanes, and its 37 floats go to LDS (9.25 KB per block).  Then wave w counts the inliers of hypotheses w, w + 4, ... over the
// pairs, 64 pairs at a time, with ballot and popcount: a count is an integer, no order of summation can change it.  Every thread walks
// the block's counts (uniform control flow); the flags of the returned hypothesis alone are written, by all 256 threads, as byte
// stores from vector registers.
#include <string.h>

#include <map>
#include <mutex>
#include <tuple>
#include <vector>

#include "pslfe_internal.h"
#include "sim3_solver_kernels.h"

#define PSL_SS_BS 256
#define PSL_SS_LDS_PAIRS 1024
#define PSL_SS_LDS_STRIDE 13
#define PSL_SS_BLOCK 64

static_assert(sizeof(PslSim3Pair) == 12 * sizeof(float), "a pair row is 12 floats");
static_assert(sizeof(PslSsHyp) == 37 * sizeof(float), "a hypothesis is 37 floats");

static __device__ const double g_ss_sctab[444] = {
#include "psl_sincostab.inc"
};

struct Sim3SolverArgs {
    const PslSim3Pair* pairs;
    const float* sig;
    const int32_t* npairs;
    int pstride, lds_pairs;
    PslSsCams K;
    const int32_t* tab;            // [pstride - min_inliers + 1] budgets by pair count
    int min_inliers, fix_scale, n_iterations;
    uint32_t seed0;
    const int32_t* start_it;
    const int32_t* best_in;
    PslSim3SolverResult* res;
    uint8_t* inliers;
};

extern __shared__ float s_ss_pairs[];

// staged pair i of the candidate into registers
__device__ __forceinline__ void ss_load(const Sim3SolverArgs& A, const float* rows, const float* sig, int lds_n, int i, float* q) {
    if (i < lds_n) {
#pragma unroll
        for (int k = 0; k < PSL_SS_STAGED_FLOATS; ++k) q[k] = s_ss_pairs[PSL_SS_LDS_STRIDE * i + k];
    } else {
        psl_ss_stage(rows + 12 * (size_t)i, sig + 2 * (size_t)i, &A.K, q);
    }
}

__device__ __noinline__ void ss_hypothesis_call(const float* P1, const float* P2, int fix_scale, PslSsHyp* H) {
    psl_ss_hypothesis(P1, P2, fix_scale, g_ss_sctab, H);
}

__device__ __forceinline__ void ss_write_result(PslSim3SolverResult* r, int status, int iterations, int ninliers, int best, const PslSsHyp* H) {
    PslSim3SolverResult o;
    o.status = status; o.iterations = iterations; o.ninliers = ninliers; o.best_inliers = best;
    for (int i = 0; i < 9; ++i) o.S12.R[i] = H ? H->R[i] : 0.f;
    for (int i = 0; i < 3; ++i) o.S12.t[i] = H ? H->t[i] : 0.f;
    o.S12.s = H ? H->s : 0.f;
    *r = o;
}

__global__ __launch_bounds__(PSL_SS_BS) void k_sim3_solve(Sim3SolverArgs A) {
    __shared__ PslSsHyp s_hyp[PSL_SS_BLOCK];
    __shared__ int s_idx[PSL_SS_BLOCK][3];
    __shared__ int s_cnt[PSL_SS_BLOCK];
    __shared__ PslRsRand s_rand;
    const int c = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = A.npairs[c];
    PslSim3SolverResult* res = A.res + c;
    const int start_it = A.start_it ? A.start_it[c] : 0, best_in = A.best_in ? A.best_in[c] : 0;
    if (n < 0 || n > A.pstride || start_it < 0 || best_in < 0) {   // uniform: an error code the set-up left there, a count the rows
        // cannot hold, or a negative state; every error path writes the status alone (the other fields 0) and no flag byte
        if (tid == 0) ss_write_result(res, n > A.pstride ? PSLFE_E_CAPACITY : PSLFE_E_INVALID, 0, 0, 0, nullptr);
        return;
    }
    uint8_t* flags = A.inliers + (size_t)c * A.pstride;
    if (n < A.min_inliers) {   // N < mRansacMinInliers: bNoMore at once (:146-150)
        for (int i = tid; i < n; i += PSL_SS_BS) flags[i] = 0;
        if (tid == 0) ss_write_result(res, 2, start_it, 0, best_in, nullptr);
        return;
    }
    const float* rows = reinterpret_cast<const float*>(A.pairs + (size_t)c * A.pstride);
    const float* sig = A.sig + 2 * (size_t)c * A.pstride;
    const int lds_n = n < A.lds_pairs ? n : A.lds_pairs;
    for (int i = tid; i < lds_n; i += PSL_SS_BS) {
        float q[PSL_SS_STAGED_FLOATS];
        psl_ss_stage(rows + 12 * (size_t)i, sig + 2 * (size_t)i, &A.K, q);
#pragma unroll
        for (int k = 0; k < PSL_SS_STAGED_FLOATS; ++k) s_ss_pairs[PSL_SS_LDS_STRIDE * i + k] = q[k];
    }
    const int max_its = A.tab[n - A.min_inliers];
    int it = start_it, best = best_in, budget = A.n_iterations;
    if (tid == 0 && it < max_its && budget > 0) {   // a call that runs no iteration draws nothing
        psl_rs_srand(&s_rand, A.seed0 + (uint32_t)c);
        for (int i = 0; i < 3 * start_it; ++i) psl_rs_rand(&s_rand);
    }
    __syncthreads();
    for (;;) {   // uniform
        int nb = max_its - it;
        if (budget < nb) nb = budget;
        if (PSL_SS_BLOCK < nb) nb = PSL_SS_BLOCK;
        if (nb <= 0) break;
        if (tid == 0)
            for (int h = 0; h < nb; ++h) psl_rs_draw<3>(&s_rand, n, s_idx[h]);
        __syncthreads();
        {
            const int h = wave * 16 + lane;
            if (lane < 16 && h < nb) {
                float q0[PSL_SS_STAGED_FLOATS], q1[PSL_SS_STAGED_FLOATS], q2[PSL_SS_STAGED_FLOATS], P1[9], P2[9];
                ss_load(A, rows, sig, lds_n, s_idx[h][0], q0);
                ss_load(A, rows, sig, lds_n, s_idx[h][1], q1);
                ss_load(A, rows, sig, lds_n, s_idx[h][2], q2);
                psl_ss_gather(q0, q1, q2, P1, P2);
                PslSsHyp H;
                ss_hypothesis_call(P1, P2, A.fix_scale, &H);
                s_hyp[h] = H;
            }
        }
        __syncthreads();
        for (int h = wave; h < nb; h += PSL_SS_BS / 64) {   // uniform in the wave
            const PslSsHyp H = s_hyp[h];
            int cnt = 0;
            for (int i0 = 0; i0 < n; i0 += 64) {
                const int i = i0 + lane;
                int in = 0;
                if (i < n) {
                    float q[PSL_SS_STAGED_FLOATS];
                    ss_load(A, rows, sig, lds_n, i, q);
                    in = psl_ss_inlier(q, &H, &A.K);
                }
                cnt += __popcll(__ballot(in));
            }
            if (lane == 0) s_cnt[h] = cnt;
        }
        __syncthreads();
        int won = -1;
        for (int h = 0; h < nb; ++h) {   // the reference's order: >= against the best, > against the minimum
            const int cnt = s_cnt[h];
            if (cnt >= best) {
                best = cnt;
                if (cnt > A.min_inliers) { won = h; break; }
            }
        }
        if (won >= 0) {
            const PslSsHyp H = s_hyp[won];
            for (int i = tid; i < n; i += PSL_SS_BS) {
                float q[PSL_SS_STAGED_FLOATS];
                ss_load(A, rows, sig, lds_n, i, q);
                flags[i] = (uint8_t)psl_ss_inlier(q, &H, &A.K);
            }
            if (tid == 0) ss_write_result(res, 1, it + won + 1, best, best, &H);
            return;
        }
        it += nb;
        budget -= nb;
    }
    for (int i = tid; i < n; i += PSL_SS_BS) flags[i] = 0;
    if (tid == 0) ss_write_result(res, it >= max_its ? 2 : 0, it, 0, best, nullptr);   // bNoMore after the loop (:203-204)
}

namespace {

int sim3_solve_check(const char* who, int ncand, int pstride, double prob, int min_inliers, int max_its, int n_iterations) {
    PSL_REQUIRE(ncand >= 0 && pstride >= 0, PSLFE_E_INVALID, "%s: ncand = %d, pstride = %d", who, ncand, pstride);
    PSL_REQUIRE(min_inliers >= 3 && max_its >= 1 && n_iterations >= 0, PSLFE_E_INVALID, "%s: min_inliers = %d, max_its = %d, n_iterations = %d", who,
                min_inliers, max_its, n_iterations);
    PSL_REQUIRE(prob > 0.0 && prob < 1.0, PSLFE_E_INVALID, "%s: prob = %g outside (0, 1)", who, prob);
    return PSLFE_OK;
}

// The budgets of the pair counts min_inliers .. pstride.  Tables are kept for the life of the library, one per set of parameters (a
// process uses one or two), so a reference handed out stays valid and an upload may read it after the call has returned.
const std::vector<int32_t>& sim3_budget_table(double prob, int min_inliers, int max_its, int pstride) {
    static std::mutex mu;
    static std::map<std::tuple<double, int, int, int>, std::vector<int32_t>> tables;
    std::lock_guard<std::mutex> lock(mu);
    std::vector<int32_t>& t = tables[std::make_tuple(prob, min_inliers, max_its, pstride)];
    if (t.empty()) {
        const int ntab = pstride >= min_inliers ? pstride - min_inliers + 1 : 0;
        t.assign((size_t)ntab + 1, 1);   // one spare entry: never empty, so an empty vector means "not built yet"
        for (int k = 0; k < ntab; ++k) t[k] = psl_ss_max_iterations(prob, min_inliers, max_its, min_inliers + k);
    }
    return t;
}

// the caller has called psl_scratch_begin when `own_scratch` is 0
int sim3_solve_launch(pslfe_ctx* ctx, const char* who, int ncand, const PslSim3Pair* d_pairs, const float* d_sigma2, const int32_t* d_npairs,
                      int pstride, const PslCamera* cam1, const PslCamera* cam2, double prob, int min_inliers, int max_its, int fix_scale,
                      uint32_t seed0, const int32_t* d_start_it, const int32_t* d_best_in, int n_iterations, PslSim3SolverResult* d_res,
                      uint8_t* d_inliers, int own_scratch) {
    Sim3SolverArgs A;
    A.pairs = d_pairs; A.sig = d_sigma2; A.npairs = d_npairs; A.pstride = pstride;
    A.lds_pairs = pstride < PSL_SS_LDS_PAIRS ? pstride : PSL_SS_LDS_PAIRS;
    A.K.fx1 = cam1->fx; A.K.fy1 = cam1->fy; A.K.cx1 = cam1->cx; A.K.cy1 = cam1->cy;
    A.K.fx2 = cam2->fx; A.K.fy2 = cam2->fy; A.K.cx2 = cam2->cx; A.K.cy2 = cam2->cy;
    A.min_inliers = min_inliers; A.fix_scale = fix_scale ? 1 : 0; A.n_iterations = n_iterations; A.seed0 = seed0;
    A.start_it = d_start_it; A.best_in = d_best_in; A.res = d_res; A.inliers = d_inliers;
    // SetRansacParameters for every pair count a candidate can have: host arithmetic with the host's libm, once per set of
    // parameters (the rounds of iterate(5) of a loop closure ask for the same table again and again), uploaded per call
    const std::vector<int32_t>& tab = sim3_budget_table(prob, min_inliers, max_its, pstride);
    if (own_scratch)
        if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    A.tab = psl_scratch_up(ctx, tab.data(), tab.size(), ctx->stream, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    const size_t lds = (size_t)A.lds_pairs * PSL_SS_LDS_STRIDE * sizeof(float);
    {
        PSL_STAGE_BEGIN(ctx, "sim3.solve");
        k_sim3_solve<<<ncand, PSL_SS_BS, lds, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "sim3.solve");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_sim3_solve_device(pslfe_ctx* ctx, int ncand, const PslSim3Pair* d_pairs, const float* d_sigma2, const int32_t* d_npairs, int pstride,
                            const PslCamera* cam1, const PslCamera* cam2, double prob, int min_inliers, int max_its, int fix_scale,
                            uint32_t seed0, const int32_t* d_start_it, const int32_t* d_best_in, int n_iterations, PslSim3SolverResult* d_res,
                            uint8_t* d_inliers) {
    static const char* who = "pslfe_sim3_solve_device";
    if (int rc = sim3_solve_check(who, ncand, pstride, prob, min_inliers, max_its, n_iterations)) return rc;
    if (ncand == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && cam1 && cam2, PSLFE_E_INVALID, "%s: NULL context or camera", who);
    PSL_REQUIRE(d_npairs && d_res, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(pstride == 0 || (d_pairs && d_sigma2 && d_inliers), PSLFE_E_INVALID, "%s: NULL pairs, sigma2 or inlier bytes with pstride = %d", who,
                pstride);
    PSL_HIP(hipSetDevice(ctx->device));
    return sim3_solve_launch(ctx, who, ncand, d_pairs, d_sigma2, d_npairs, pstride, cam1, cam2, prob, min_inliers, max_its, fix_scale, seed0,
                             d_start_it, d_best_in, n_iterations, d_res, d_inliers, 1);
}

int pslfe_sim3_solve(pslfe_ctx* ctx, const PslSim3Pair* pairs, const float* sigma2, int npairs, const PslCamera* cam1, const PslCamera* cam2,
                     double prob, int min_inliers, int max_its, int fix_scale, uint32_t seed, int start_it, int best_in, int n_iterations,
                     PslSim3SolverResult* res, uint8_t* inliers) {
    static const char* who = "pslfe_sim3_solve";
    PSL_REQUIRE(npairs >= 0 && start_it >= 0 && best_in >= 0, PSLFE_E_INVALID, "%s: npairs = %d, start_it = %d, best_in = %d", who, npairs, start_it,
                best_in);
    if (int rc = sim3_solve_check(who, 1, npairs, prob, min_inliers, max_its, n_iterations)) return rc;
    PSL_REQUIRE(ctx && cam1 && cam2 && res, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(npairs == 0 || (pairs && sigma2 && inliers), PSLFE_E_INVALID, "%s: NULL pairs, sigma2 or inlier bytes with npairs = %d", who, npairs);
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int32_t n32 = npairs, s32 = start_it, b32 = best_in;
    const PslSim3Pair* d_pairs = psl_scratch_up(ctx, npairs ? pairs : nullptr, (size_t)npairs, st, &e);
    const float* d_sig = psl_scratch_up(ctx, npairs ? sigma2 : nullptr, 2 * (size_t)npairs, st, &e);
    const int32_t* d_n = psl_scratch_up(ctx, &n32, 1, st, &e);
    const int32_t* d_s = psl_scratch_up(ctx, &s32, 1, st, &e);
    const int32_t* d_b = psl_scratch_up(ctx, &b32, 1, st, &e);
    PslSim3SolverResult* d_res = psl_scratch_up(ctx, (const PslSim3SolverResult*)nullptr, 1, st, &e);
    uint8_t* d_inl = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)npairs, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    if (int rc = sim3_solve_launch(ctx, who, 1, d_pairs, d_sig, d_n, npairs, cam1, cam2, prob, min_inliers, max_its, fix_scale, seed, d_s, d_b,
                                   n_iterations, d_res, d_inl, 0))
        return rc;
    PSL_HIP(hipMemcpyAsync(res, d_res, sizeof(PslSim3SolverResult), hipMemcpyDeviceToHost, st));
    if (npairs) PSL_HIP(hipMemcpyAsync(inliers, d_inl, (size_t)npairs, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

}  // extern "C"
