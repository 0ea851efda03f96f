// libpslfe: Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:37-237; the calls of
// Tracking::CreateInitialMapMonocular src/Tracking.cc:782 and LoopClosing::RunGlobalBundleAdjustment src/LoopClosing.cc:650): ONE
// problem spread over the whole device.  Product code.
// Who owns what.  ba_kernels.h holds the arithmetic (the edges, the quadratic form, the Schur terms, the landmark inverse, the
// back-substitution of the points), lm_kernels.h the Levenberg loop psl_lm_levenberg, gba_kernels.h the driver psl_gba_optimize with
// its `Problem` and the steps that have a form of their own at this size, lm_grid.h the executor PslLmGrid (a step = a plain
// stream-ordered launch over the device, a decision = a small read-back) and the panel kernels of the dense solve.  This file owns
// the handle, the checks and the entry points.  tools/dropin/gba_main.cpp runs the same driver on PslLmSerial.
//
// A call.  The edge rows are read back once: the row check (psl_ba_check_rows), the four stable counting sorts and the duplicate
// check (psl_ba_lists_host) run on the host, on the text the one-core loop uses, and the offsets and lists go up to the workspace
// (24 bytes per edge down, 16 up).  Then psl_gba_optimize drives the loop from the host: per trial 5 read-backs
// (three solve flags, the candidate's chi2, computeScale), per iteration one more (the chi2; in iteration 0 also lambda), per call
// two (F, the included points).  The call returns when the outputs are written.
#include <string.h>

#include <vector>

#include "pslfe_internal.h"
#include "lm_grid.h"

static_assert(sizeof(PslGbaInfo) == 40, "global BA POD");

// the sin / cos table of psl_sincos_glibc.h; pslfe_gba_create copies it into the handle's own device buffer
static const double k_gba_sctab[444] = {
#include "psl_sincostab.inc"
};

struct pslfe_gba {
    pslfe_ctx* ctx = nullptr;
    int ckf = 0, cmp = 0, ced = 0;
    PslDeviceBuffers bufs;
    char* d_ws = nullptr;
    double* d_sum = nullptr;
    PslGbaWs G;                       // the views of d_ws
    double* d_sctab = nullptr;        // [444]
    // the host side of the checks and the lists
    std::vector<PslBaEdge> h_ed;
    std::vector<int32_t> h_koff, h_poff, h_cursor, h_klist, h_plist, h_kplist, h_pklist;
};

// outputs = inputs, not_included = 0: a refused problem
static int gba_copy_through(pslfe_ctx* ctx, const PslBaKeyFrame* d_kf, int nkf, const PslMapPointGeom* d_mp, int nmp, PslBaKeyFrame* d_kf_out,
                            PslMapPointGeom* d_mp_out, uint8_t* d_not_included) {
    if (nkf && d_kf_out != d_kf) PSL_HIP(hipMemcpyAsync(d_kf_out, d_kf, (size_t)nkf * sizeof(PslBaKeyFrame), hipMemcpyDeviceToDevice, ctx->stream));
    if (nmp && d_mp_out != d_mp) PSL_HIP(hipMemcpyAsync(d_mp_out, d_mp, (size_t)nmp * sizeof(PslMapPointGeom), hipMemcpyDeviceToDevice, ctx->stream));
    if (nmp) PSL_HIP(hipMemsetAsync(d_not_included, 0, (size_t)nmp, ctx->stream));
    PSL_HIP(hipStreamSynchronize(ctx->stream));
    return PSLFE_OK;
}

// The row check, the four stable counting sorts and the duplicate check on the edge rows in g->h_ed, with the text the one-core loop
// uses (psl_ba_check_rows, psl_ba_lists_host): PSLFE_OK and the offsets and lists in the handle's host vectors, or PSLFE_E_INVALID.
// Host text: ba_kernels.h shows psl_ba_lists_host to the host pass only, so the device pass sees the declaration alone
// (not static: a static function without a definition draws a warning there).
int psl_gba_host_lists(pslfe_gba* g, int nkf, int nmp, int nedges);
#if !defined(__HIP_DEVICE_COMPILE__)
int psl_gba_host_lists(pslfe_gba* g, int nkf, int nmp, int nedges) {
    if (int rc = psl_ba_check_rows(g->h_ed.data(), nkf, nmp, nedges)) return rc;
    const size_t cv = (size_t)(nkf > nmp ? nkf : nmp) + 1;
    g->h_koff.assign((size_t)nkf + 1, 0); g->h_poff.assign((size_t)nmp + 1, 0); g->h_cursor.assign(cv, 0);
    g->h_klist.resize((size_t)nedges); g->h_plist.resize((size_t)nedges); g->h_kplist.resize((size_t)nedges); g->h_pklist.resize((size_t)nedges);
    PslBaWs H = {};
    H.ed = g->h_ed.data(); H.nkf = nkf; H.nmp = nmp; H.ne = nedges;
    H.koff = g->h_koff.data(); H.poff = g->h_poff.data(); H.cursor = g->h_cursor.data();
    H.klist = g->h_klist.data(); H.plist = g->h_plist.data(); H.kplist = g->h_kplist.data(); H.pklist = g->h_pklist.data();
    return psl_ba_lists_host(H);
}
#endif

extern "C" {

int pslfe_gba_create(pslfe_ctx* ctx, int max_keyframes, int max_points, int max_edges, pslfe_gba** out) {
    static const char* who = "pslfe_gba_create";
    PSL_REQUIRE(ctx && out, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(max_keyframes >= 1 && max_points >= 1 && max_edges >= 1, PSLFE_E_INVALID, "%s: max_keyframes = %d, max_points = %d, max_edges = %d", who,
                max_keyframes, max_points, max_edges);
    PSL_REQUIRE(max_keyframes <= 4096, PSLFE_E_INVALID, "%s: max_keyframes = %d (S has 36 max_keyframes^2 doubles)", who, max_keyframes);
    // every index of a step is an int: nkf + nmp + ne, 9 nmp, 6 nkf + 3 nmp
    PSL_REQUIRE(max_points <= (1 << 26) && max_edges <= (1 << 26), PSLFE_E_INVALID, "%s: max_points = %d, max_edges = %d (at most 2^26 each)", who,
                max_points, max_edges);
    PSL_HIP(hipSetDevice(ctx->device));
    pslfe_gba* g = new pslfe_gba;
    g->ctx = ctx; g->ckf = max_keyframes; g->cmp = max_points; g->ced = max_edges;
    const size_t bytes = psl_gba_carve(nullptr, max_keyframes, max_points, max_edges, &g->G);
    g->bufs.alloc(g->d_ws, bytes, "workspace");
    g->bufs.alloc(g->d_sum, 1, "sum");
    g->bufs.alloc(g->d_sctab, 444, "sin / cos table");
    if (int rc = g->bufs.check(who)) { delete g; return rc; }
    psl_gba_carve(g->d_ws, max_keyframes, max_points, max_edges, &g->G);
    hipError_t e = hipMemcpyAsync(g->d_sctab, k_gba_sctab, sizeof(k_gba_sctab), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        pslfe_set_error("%s: uploading the sin / cos table: %s", who, hipGetErrorString(e));
        delete g;
        return PSLFE_E_HIP;
    }
    *out = g;
    return PSLFE_OK;
}

void pslfe_gba_destroy(pslfe_gba* gba) {
    if (!gba) return;
    (void)hipSetDevice(gba->ctx->device);
    (void)hipStreamSynchronize(gba->ctx->stream);
    delete gba;
}

int pslfe_gba_optimize_device(pslfe_gba* gba, const PslBaKeyFrame* d_kf, int nkf, const PslMapPointGeom* d_mp, int nmp, const PslBaEdge* d_edges,
                              int nedges, const PslCamera* cam, int iterations, int robust, PslBaKeyFrame* d_kf_out, PslMapPointGeom* d_mp_out,
                              uint8_t* d_not_included, PslGbaInfo* info) {
    static const char* who = "pslfe_gba_optimize_device";
    PSL_REQUIRE(nkf >= 0 && nmp >= 0 && nedges >= 0 && iterations >= 1 && robust >= 0 && robust <= 1, PSLFE_E_INVALID,
                "%s: nkf = %d, nmp = %d, nedges = %d, iterations = %d (>= 1), robust = %d (0..1)", who, nkf, nmp, nedges, iterations, robust);
    PSL_REQUIRE(gba && cam && info, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE((nkf == 0 || (d_kf && d_kf_out)) && (nmp == 0 || (d_mp && d_mp_out && d_not_included)) && (nedges == 0 || d_edges), PSLFE_E_INVALID,
                "%s: NULL array with a non-zero count", who);
    pslfe_ctx* ctx = gba->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    memset(info, 0, sizeof(*info));
    if (nkf > gba->ckf || nmp > gba->cmp || nedges > gba->ced) {
        info->status = PSLFE_E_CAPACITY;
        if (int rc = gba_copy_through(ctx, d_kf, nkf, d_mp, nmp, d_kf_out, d_mp_out, d_not_included)) return rc;
        pslfe_set_error("%s: nkf = %d, nmp = %d, nedges = %d above the handle's caps %d, %d, %d", who, nkf, nmp, nedges, gba->ckf, gba->cmp, gba->ced);
        return PSLFE_E_CAPACITY;
    }
    // the checks and the lists
    PslGbaWs G = gba->G;
    PslBaWs& W = G.B;
    W.kf = d_kf; W.mp = d_mp; W.ed = d_edges;
    W.nkf = nkf; W.nmp = nmp; W.ne = nedges;
    W.K.fx = (double)cam->fx; W.K.fy = (double)cam->fy; W.K.cx = (double)cam->cx; W.K.cy = (double)cam->cy; W.K.bf = (double)cam->bf;
    W.sctab = gba->d_sctab;
    gba->h_ed.resize((size_t)nedges);
    if (nedges) PSL_HIP(hipMemcpyAsync(gba->h_ed.data(), d_edges, (size_t)nedges * sizeof(PslBaEdge), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    const int status = psl_gba_host_lists(gba, nkf, nmp, nedges);
    if (status != PSLFE_OK) {
        info->status = status;
        if (int rc = gba_copy_through(ctx, d_kf, nkf, d_mp, nmp, d_kf_out, d_mp_out, d_not_included)) return rc;
        pslfe_set_error("%s: the problem was refused with %d (an edge outside the problem or a duplicate pair)", who, status);
        return status;
    }
    PSL_HIP(hipMemcpyAsync(W.koff, gba->h_koff.data(), ((size_t)nkf + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    PSL_HIP(hipMemcpyAsync(W.poff, gba->h_poff.data(), ((size_t)nmp + 1) * sizeof(int32_t), hipMemcpyHostToDevice, st));
    if (nedges) {
        const size_t lb = (size_t)nedges * sizeof(int32_t);
        PSL_HIP(hipMemcpyAsync(W.klist, gba->h_klist.data(), lb, hipMemcpyHostToDevice, st));
        PSL_HIP(hipMemcpyAsync(W.plist, gba->h_plist.data(), lb, hipMemcpyHostToDevice, st));
        PSL_HIP(hipMemcpyAsync(W.kplist, gba->h_kplist.data(), lb, hipMemcpyHostToDevice, st));
        PSL_HIP(hipMemcpyAsync(W.pklist, gba->h_pklist.data(), lb, hipMemcpyHostToDevice, st));
    }
    PslLmGrid X = {st, gba->d_sum, hipSuccess, 0, 0};
    PslGbaResult R;
    {
        PSL_STAGE_BEGIN(ctx, "gba.optimize");
        R = psl_gba_optimize(X, G, iterations, robust, d_kf_out, d_mp_out, d_not_included);
        PSL_STAGE_END(ctx, "gba.optimize");
    }
    X.note(hipStreamSynchronize(st));
    PSL_REQUIRE(X.err == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(X.err));
    info->status = PSLFE_OK;
    info->iterations = R.iterations; info->free_keyframes = R.free_keyframes; info->included_points = R.included_points;
    info->chi2_start = R.chi2_start; info->chi2_end = R.chi2_end; info->lambda = R.lambda;
    return PSLFE_OK;
}

int pslfe_gba_optimize(pslfe_gba* gba, const PslBaKeyFrame* kf, int nkf, const PslMapPointGeom* mp, int nmp, const PslBaEdge* edges, int nedges,
                       const PslCamera* cam, int iterations, int robust, PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out, uint8_t* not_included,
                       PslGbaInfo* info) {
    static const char* who = "pslfe_gba_optimize";
    PSL_REQUIRE(nkf >= 0 && nmp >= 0 && nedges >= 0 && iterations >= 1 && robust >= 0 && robust <= 1, PSLFE_E_INVALID,
                "%s: nkf = %d, nmp = %d, nedges = %d, iterations = %d (>= 1), robust = %d (0..1)", who, nkf, nmp, nedges, iterations, robust);
    PSL_REQUIRE(gba && cam && info, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE((nkf == 0 || (kf && kf_out)) && (nmp == 0 || (mp && mp_out && not_included)) && (nedges == 0 || edges), PSLFE_E_INVALID,
                "%s: NULL array with a non-zero count", who);
    pslfe_ctx* ctx = gba->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    PslBaKeyFrame* d_kf = psl_scratch_up(ctx, nkf ? kf : nullptr, (size_t)nkf, st, &e);
    PslMapPointGeom* d_mp = psl_scratch_up(ctx, nmp ? mp : nullptr, (size_t)nmp, st, &e);
    PslBaEdge* d_ed = psl_scratch_up(ctx, nedges ? edges : nullptr, (size_t)nedges, st, &e);
    uint8_t* d_ni = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)nmp, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    const int rc = pslfe_gba_optimize_device(gba, d_kf, nkf, d_mp, nmp, d_ed, nedges, cam, iterations, robust, d_kf, d_mp, d_ni, info);
    if (rc != PSLFE_OK && rc != PSLFE_E_CAPACITY && rc != PSLFE_E_INVALID) return rc;
    if (nkf) PSL_HIP(hipMemcpyAsync(kf_out, d_kf, (size_t)nkf * sizeof(PslBaKeyFrame), hipMemcpyDeviceToHost, st));
    if (nmp) PSL_HIP(hipMemcpyAsync(mp_out, d_mp, (size_t)nmp * sizeof(PslMapPointGeom), hipMemcpyDeviceToHost, st));
    if (nmp) PSL_HIP(hipMemcpyAsync(not_included, d_ni, (size_t)nmp, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return rc;
}

}  // extern "C"
