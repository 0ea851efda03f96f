// libpslfe: Optimizer::OptimizeEssentialGraph (src/Optimizer.cc:2536-2799) for K graphs in one launch.  Product code.
// Who owns what.  essential_kernels.h holds everything that is arithmetic or a decision: the measurements, Sim3::log, the edge and
// its numeric Jacobian, the blocks, the envelope LDLt, the `Problem` of the Levenberg driver psl_lm_levenberg (lm_kernels.h), the
// poses and the points, and the checks of the rows, written once over an executor (the contract: lm_kernels.h); the host loop of
// tools/dropin/essential_main.cpp runs the same text on one core.  This file owns the handle and the entry points; the executor of
// a workgroup is PslLmWorkgroup of lm_device.h.  Conventions: include/pslfe.h above pslfe_eg_optimize_device.
//
// k_eg_optimize: one launch, one resident workgroup of 256 threads per graph through the lists, every iteration and every trial.
// The executor spreads the indices of a step over the threads (thread = (keyframe, column, sign) for the perturbed estimates;
// thread = (edge, half, column) for the 28 + 1 error evaluations of an edge; thread = (block, entry) walking the keyframe's items in
// order for H and b; thread = row for a column of the LDLt; thread = keyframe for the candidates and the poses; thread = point for
// the correction) and ends the step with a barrier; sum256 is the ordered reduction psl_lm_reduce of lm_device.h.  Control flow is
// uniform: every decision is taken from values all threads read back after a barrier.
//
// Workgroup size.  256 threads = 4 waves: the ordered reduction is defined on 256 partial sums.  The workspace (per edge 105
// doubles of error and Jacobians, per keyframe 28 perturbed estimates, the two envelopes) lives in HBM / L2.  The kernel is latency
// bound by construction: 7 F columns of the LDLt with a barrier each, and the two substitutions on one thread, per trial; a
// single graph uses one CU, and the device fills only when K reaches the CU count (profiles/essential_graph_bench.json,
// profiles/essential_graph_codegen.txt).
#include <string.h>

#include "pslfe_internal.h"
#include "essential_kernels.h"
#include "lm_device.h"

#define PSL_EG_BS PSL_LM_LANES

static_assert(sizeof(PslEgKeyFrame) == 136 && sizeof(PslEgEdge) == 12 && sizeof(PslEgInfo) == 40 && sizeof(PslS3) == 64, "essential graph PODs");
static_assert(PSL_EG_BS == 4 * PSL_LM_GROUP, "four waves of 64");

__device__ const double g_eg_sctab[444] = {
#include "psl_sincostab.inc"
};

struct pslfe_eg {
    pslfe_ctx* ctx = nullptr;
    int max_graphs = 0, ckf = 0, ced = 0, cmp = 0;
    size_t cenv = 0, ws_stride = 0;
    PslDeviceBuffers bufs;
    char* d_ws = nullptr;   // [max_graphs][ws_stride]
};

struct EgArgs {
    const PslEgKeyFrame* kf;
    const int32_t* kf_off;
    const PslEgEdge* ed;
    const int32_t* ed_off;
    const PslMapPointGeom* mp;
    const int32_t* mp_ref;
    const int32_t* mp_off;
    int fix_scale, ckf, ced, cmp;
    size_t cenv;
    char* ws;
    size_t ws_stride;
    PslPose* pose_out;
    double* S_out;
    PslMapPointGeom* mp_out;
    PslEgInfo* info;
};

__global__ __launch_bounds__(PSL_EG_BS) void k_eg_optimize(EgArgs A) {
    __shared__ double s_red[2 * 4];
    const int k = blockIdx.x;
    const int k0 = A.kf_off[k], k1 = A.kf_off[k + 1], e0 = A.ed_off[k], e1 = A.ed_off[k + 1], p0 = A.mp_off[k], p1 = A.mp_off[k + 1];
    PslEgWs W;
    int have = 1, code = PSLFE_OK;
    if (k0 < 0 || e0 < 0 || p0 < 0 || k1 < k0 || e1 < e0 || p1 < p0) { have = 0; code = PSLFE_E_INVALID; }
    else if (k1 - k0 > A.ckf || e1 - e0 > A.ced || p1 - p0 > A.cmp) code = PSLFE_E_CAPACITY;
    psl_eg_carve(A.ws + (size_t)k * A.ws_stride, A.ckf, A.ced, A.cenv, &W);
    W.kf = A.kf + (have ? k0 : 0); W.ed = A.ed + (have ? e0 : 0); W.mp = A.mp + (have ? p0 : 0); W.mp_ref = A.mp_ref + (have ? p0 : 0);
    W.nkf = have ? k1 - k0 : 0; W.ne = have ? e1 - e0 : 0; W.nmp = have ? p1 - p0 : 0;
    W.fix_scale = A.fix_scale;
    W.sctab = g_eg_sctab;
    PslLmWorkgroup X = {s_red, 0};
    psl_eg_run(X, W, have, code, A.cenv, A.pose_out + (have ? k0 : 0), A.S_out + 8 * (size_t)(have ? k0 : 0), A.mp_out + (have ? p0 : 0), A.info + k);
}

extern "C" {

int pslfe_eg_create(pslfe_ctx* ctx, int max_graphs, int max_keyframes, int max_edges, int max_points, int64_t max_envelope, pslfe_eg** out) {
    static const char* who = "pslfe_eg_create";
    PSL_REQUIRE(ctx && out, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(max_graphs >= 1 && max_keyframes >= 1 && max_edges >= 1 && max_points >= 1 && max_envelope >= 1, PSLFE_E_INVALID,
                "%s: max_graphs = %d, max_keyframes = %d, max_edges = %d, max_points = %d, max_envelope = %lld", who, max_graphs, max_keyframes,
                max_edges, max_points, (long long)max_envelope);
    PSL_REQUIRE(max_keyframes <= (1 << 20) && max_edges <= (1 << 24), PSLFE_E_INVALID, "%s: max_keyframes = %d, max_edges = %d", who, max_keyframes,
                max_edges);
    PSL_HIP(hipSetDevice(ctx->device));
    pslfe_eg* g = new pslfe_eg;
    g->ctx = ctx; g->max_graphs = max_graphs; g->ckf = max_keyframes; g->ced = max_edges; g->cmp = max_points; g->cenv = (size_t)max_envelope;
    PslEgWs W;
    g->ws_stride = psl_align_up(psl_eg_carve(nullptr, max_keyframes, max_edges, g->cenv, &W), 256);
    g->bufs.alloc(g->d_ws, g->ws_stride * (size_t)max_graphs, "workspaces");
    if (int rc = g->bufs.check(who)) { delete g; return rc; }
    *out = g;
    return PSLFE_OK;
}

void pslfe_eg_destroy(pslfe_eg* eg) {
    if (!eg) return;
    (void)hipSetDevice(eg->ctx->device);
    (void)hipStreamSynchronize(eg->ctx->stream);
    delete eg;
}

int pslfe_eg_optimize_device(pslfe_eg* eg, int K, const PslEgKeyFrame* d_kf, const int32_t* d_kf_off, const PslEgEdge* d_edges,
                             const int32_t* d_edge_off, const PslMapPointGeom* d_mp, const int32_t* d_mp_ref, const int32_t* d_mp_off,
                             int fix_scale, PslPose* d_pose_out, double* d_S_out, PslMapPointGeom* d_mp_out, PslEgInfo* d_info) {
    static const char* who = "pslfe_eg_optimize_device";
    PSL_REQUIRE(K >= 0, PSLFE_E_INVALID, "%s: K = %d", who, K);
    if (K == 0) return PSLFE_OK;
    PSL_REQUIRE(eg, PSLFE_E_INVALID, "%s: NULL handle", who);
    PSL_REQUIRE(K <= eg->max_graphs, PSLFE_E_INVALID, "%s: K = %d above max_graphs = %d", who, K, eg->max_graphs);
    PSL_REQUIRE(d_kf && d_kf_off && d_edges && d_edge_off && d_mp && d_mp_ref && d_mp_off && d_pose_out && d_S_out && d_mp_out && d_info,
                PSLFE_E_INVALID, "%s: NULL array", who);
    pslfe_ctx* ctx = eg->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    EgArgs A = {};
    A.kf = d_kf; A.kf_off = d_kf_off; A.ed = d_edges; A.ed_off = d_edge_off; A.mp = d_mp; A.mp_ref = d_mp_ref; A.mp_off = d_mp_off;
    A.fix_scale = fix_scale ? 1 : 0; A.ckf = eg->ckf; A.ced = eg->ced; A.cmp = eg->cmp; A.cenv = eg->cenv;
    A.ws = eg->d_ws; A.ws_stride = eg->ws_stride;
    A.pose_out = d_pose_out; A.S_out = d_S_out; A.mp_out = d_mp_out; A.info = d_info;
    {
        PSL_STAGE_BEGIN(ctx, "eg.optimize");
        k_eg_optimize<<<K, PSL_EG_BS, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "eg.optimize");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int pslfe_eg_optimize(pslfe_eg* eg, const PslEgKeyFrame* kf, int nkf, const PslEgEdge* edges, int nedges, const PslMapPointGeom* mp,
                      const int32_t* mp_ref, int nmp, int fix_scale, PslPose* pose_out, double* S_out, PslMapPointGeom* mp_out, PslEgInfo* info) {
    static const char* who = "pslfe_eg_optimize";
    PSL_REQUIRE(nkf >= 0 && nedges >= 0 && nmp >= 0, PSLFE_E_INVALID, "%s: nkf = %d, nedges = %d, nmp = %d", who, nkf, nedges, nmp);
    PSL_REQUIRE(eg && info, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE((nkf == 0 || (kf && pose_out && S_out)) && (nedges == 0 || edges) && (nmp == 0 || (mp && mp_ref && mp_out)), PSLFE_E_INVALID,
                "%s: NULL array with a non-zero count", who);
    pslfe_ctx* ctx = eg->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int32_t koff[2] = {0, nkf}, eoff[2] = {0, nedges}, poff[2] = {0, nmp};
    // a zero count still gets one row of scratch: the device form takes no NULL array
    PslEgKeyFrame* d_kf = psl_scratch_up(ctx, nkf ? kf : nullptr, (size_t)(nkf ? nkf : 1), st, &e);
    PslEgEdge* d_ed = psl_scratch_up(ctx, nedges ? edges : nullptr, (size_t)(nedges ? nedges : 1), st, &e);
    PslMapPointGeom* d_mp = psl_scratch_up(ctx, nmp ? mp : nullptr, (size_t)(nmp ? nmp : 1), st, &e);
    int32_t* d_ref = psl_scratch_up(ctx, nmp ? mp_ref : nullptr, (size_t)(nmp ? nmp : 1), st, &e);
    const int32_t* d_koff = psl_scratch_up(ctx, koff, 2, st, &e);
    const int32_t* d_eoff = psl_scratch_up(ctx, eoff, 2, st, &e);
    const int32_t* d_poff = psl_scratch_up(ctx, poff, 2, st, &e);
    PslPose* d_pose = psl_scratch_up(ctx, (const PslPose*)nullptr, (size_t)(nkf ? nkf : 1), st, &e);
    double* d_S = psl_scratch_up(ctx, (const double*)nullptr, 8 * (size_t)(nkf ? nkf : 1), st, &e);
    PslEgInfo* d_info = psl_scratch_up(ctx, (const PslEgInfo*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    if (int rc = pslfe_eg_optimize_device(eg, 1, d_kf, d_koff, d_ed, d_eoff, d_mp, d_ref, d_poff, fix_scale, d_pose, d_S, d_mp, d_info)) return rc;
    PSL_HIP(hipMemcpyAsync(info, d_info, sizeof(PslEgInfo), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    if (info->status < 0) {   // refused: the outputs are the inputs; no pose row
        for (int v = 0; v < nkf; ++v) memcpy(S_out + 8 * (size_t)v, kf[v].Scw, 8 * sizeof(double));
        if (nmp && mp_out != mp) memcpy(mp_out, mp, (size_t)nmp * sizeof(PslMapPointGeom));
        pslfe_set_error("%s: the graph was refused with %d (%s)", who, info->status,
                        info->status == PSLFE_E_CAPACITY ? "a count or the envelope above the handle's caps" : "an edge or a point outside the graph");
        return info->status;
    }
    if (nkf) PSL_HIP(hipMemcpyAsync(pose_out, d_pose, (size_t)nkf * sizeof(PslPose), hipMemcpyDeviceToHost, st));
    if (nkf) PSL_HIP(hipMemcpyAsync(S_out, d_S, 8 * (size_t)nkf * sizeof(double), hipMemcpyDeviceToHost, st));
    if (nmp) PSL_HIP(hipMemcpyAsync(mp_out, d_mp, (size_t)nmp * sizeof(PslMapPointGeom), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

}  // extern "C"
