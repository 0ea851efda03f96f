// libpslfe: projection of map lines into a frame, up to the line window search of pslfe_linematch.hip.  Product code.
// Reference behaviour reproduced:
//   Frame::isInFrustum(MapLine*, viewingCosLimit)                         src/Frame.cc:828-904
//   MapLine::PredictScale, Get{Min,Max}DistanceInvariance                 add_src/MapLine.cpp:369-390
//   LSDmatcher::SearchByProjection(cur,last,th) up to the window search   add_src/LSDmatcher.cpp:112-155
//   LSDmatcher::SearchByProjection(F,MLs,..,th) up to the window search   add_src/LSDmatcher.cpp:260-289, RadiusByViewingCos :986-992
//
// The cv::Mat conventions are those of the point projections; the frame column of DESIGN.md §5.0h lists what differs from the line Fuse.
//
// One workgroup per frame or pair (blockIdx.y): thread t handles lines t, t + 256, ... and the emitted rows are compacted in line
// order by a workgroup scan, so the matcher's first-come-first-served order is the reference's loop order.
#include <limits.h>
#include <string.h>

#include "pslfe_internal.h"
#include "psl_device_math.h"
#define PSL_F64_QUAL __host__ __device__ static inline
#include "psl_f64math.h"

#include "proj_kernels.h"
#include "kf_project.h"

#define PSL_LPROJ_BS 256

namespace {

struct LineView {
    float u1, v1, u2, v2, viewCos;
    int level;
};

// Frame::isInFrustum(pML, limit) src/Frame.cc:828-904 against pose T with camera centre Ow.
__device__ bool psl_line_in_frustum(const double* sp, const double* ep, const double* nrm, float min_dist, float max_dist, const PslPose& T,
                                    const float* Ow, const ProjParams& P, float limit, LineView* out) {
    const PslCamera& C = P.cam;
    const float SP[3] = {(float)sp[0], (float)sp[1], (float)sp[2]};
    const float EP[3] = {(float)ep[0], (float)ep[1], (float)ep[2]};
    float SPc[3], EPc[3];
    psl_pose_mul(T.R, T.t, SP[0], SP[1], SP[2], SPc);
    psl_pose_mul(T.R, T.t, EP[0], EP[1], EP[2], EPc);
    const float SPcX = SPc[0], SPcY = SPc[1], SPcZ = SPc[2], EPcX = EPc[0], EPcY = EPc[1], EPcZ = EPc[2];
    if (SPcZ < 0.0f || EPcZ < 0.0f) return false;
    if (!(SPcZ > 0.0f) || !(EPcZ > 0.0f)) return false;  // z == 0 or NaN: stated outcome, not in view
    const float invz1 = PSL_FDIV(1.0f, SPcZ);
    const float u1 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fx, SPcX), invz1), C.cx);
    const float v1 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fy, SPcY), invz1), C.cy);
    if (!(u1 >= P.minX && u1 <= P.maxX)) return false;
    if (!(v1 >= P.minY && v1 <= P.maxY)) return false;
    const float invz2 = PSL_FDIV(1.0f, EPcZ);
    const float u2 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fx, EPcX), invz2), C.cx);
    const float v2 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fy, EPcY), invz2), C.cy);
    if (!(u2 >= P.minX && u2 <= P.maxX)) return false;
    if (!(v2 >= P.minY && v2 <= P.maxY)) return false;
    const float maxD = PSL_FMUL(1.2f, max_dist), minD = PSL_FMUL(0.8f, min_dist);
    float OM[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) OM[k] = PSL_FSUB(psl_half_sum(SP[k], EP[k]), Ow[k]);
    const float dist = psl_norm3(OM[0], OM[1], OM[2]);
    if (!(dist >= minD && dist <= maxD)) return false;
    const double dot = psl_dot3(OM[0], OM[1], OM[2], (float)nrm[0], (float)nrm[1], (float)nrm[2]);
    const float viewCos = (float)PSL_DDIV(dot, (double)dist);
    if (!(viewCos >= limit)) return false;
    out->u1 = u1; out->v1 = v1; out->u2 = u2; out->v2 = v2;
    out->viewCos = viewCos;
    out->level = psl_line_level(PSL_FDIV(max_dist, dist), P.log_scale_factor);
    return true;
}

struct LineFrustumArgs {
    const PslPose* Tcw;
    const PslMapLineGeom* ml;
    const uint8_t* mldesc;
    const int32_t* nml;
    int mlstride;
    PslLineQuery* q;
    uint8_t* qdesc;
    int32_t* owner;
    int32_t* nq;
    int qstride;
    uint8_t* inview;
    int32_t* level;
    float* viewcos;
};

__global__ __launch_bounds__(PSL_LPROJ_BS) void k_line_project_frustum(LineFrustumArgs A, ProjParams P) {
    __shared__ int s_wave[PSL_LPROJ_BS / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    const size_t base = (size_t)f * A.mlstride;
    const int n = min(A.nml[f], A.mlstride);
    const PslPose T = A.Tcw[f];
    float Ow[3];
    psl_centre(T, Ow);
    int written = 0;
    for (int j0 = 0; j0 < n; j0 += PSL_LPROJ_BS) {
        const int j = j0 + tid;
        bool emit = false;
        PslLineQuery row;
        LineView V;
        if (j < n) {
            const PslMapLineGeom& G = A.ml[base + j];
            emit = psl_line_in_frustum(G.sp, G.ep, G.normal, G.min_dist, G.max_dist, T, Ow, P, P.view_cos_limit, &V);
            if (emit) {
                float r = (double)V.viewCos > 0.998 ? 5.0f : 8.0f;
                if (P.th != 1.0f) r = PSL_FMUL(r, P.th);
                row.x1 = V.u1; row.y1 = V.v1; row.x2 = V.u2; row.y2 = V.v2;
                row.radius = r;
                row.th_cos = 0.998f;
                row.vx = 0.f; row.vy = 0.f; row.length = 0.f;
                row.blocks = 1;
                row.wdir[0] = G.normal[0]; row.wdir[1] = G.normal[1]; row.wdir[2] = G.normal[2];
            }
            if (A.inview) A.inview[base + j] = emit ? 1 : 0;
            if (A.level) A.level[base + j] = emit ? V.level : -1;
            if (A.viewcos) A.viewcos[base + j] = emit ? V.viewCos : 0.f;
        }
        int total;
        const int q = written + psl_wg_compact<PSL_LPROJ_BS>(emit, s_wave, &total);
        if (emit && q < A.qstride) {
            const size_t r = (size_t)f * A.qstride + q;
            A.q[r] = row;
            psl_copy_desc(A.qdesc + r * 32, A.mldesc + (base + j) * 32);
            if (A.owner) A.owner[r] = j;
        }
        written += total;
    }
    if (tid == 0) A.nq[f] = written;
}

struct LineLastArgs {
    const PslKeyLine* kls;
    const uint8_t* ldesc;
    const int32_t* nkl;
    int kl_stride;
    const PslLastLine* lines;
    const uint8_t* mldesc;
    const PslPose* Tcw;
    PslLineQuery* q;
    uint8_t* qdesc;
    int32_t* owner;
    int32_t* nq;
    int qstride;
};

__global__ __launch_bounds__(PSL_LPROJ_BS) void k_line_project_last(LineLastArgs A, ProjParams P) {
    __shared__ int s_wave[PSL_LPROJ_BS / 64];
    const int p = blockIdx.y, tid = threadIdx.x;
    const size_t base = (size_t)p * A.kl_stride;
    const int n = min(A.nkl[p], A.kl_stride);
    const PslPose T = A.Tcw[p];
    float Ow[3];
    psl_centre(T, Ow);
    int written = 0;
    for (int i0 = 0; i0 < n; i0 += PSL_LPROJ_BS) {
        const int i = i0 + tid;
        bool emit = false;
        PslLineQuery row;
        if (i < n) {
            const PslLastLine& L = A.lines[base + i];
            LineView V;
            if ((L.state & 3) != 0 && !(L.state & 8) &&
                psl_line_in_frustum(L.sp, L.ep, L.normal, L.min_dist, L.max_dist, T, Ow, P, 0.5f, &V)) {
                const PslKeyLine& kl = A.kls[base + i];
                row.x1 = V.u1; row.y1 = V.v1; row.x2 = V.u2; row.y2 = V.v2;
                row.radius = P.th;
                row.th_cos = 0.96f;
                row.vx = PSL_FSUB(kl.ePointInOctaveX, kl.sPointInOctaveX);
                row.vy = PSL_FSUB(kl.ePointInOctaveY, kl.sPointInOctaveY);
                row.length = kl.lineLength;
                row.blocks = (L.state & 3) == 2;
                row.wdir[0] = 0.0; row.wdir[1] = 0.0; row.wdir[2] = 0.0;
                emit = true;
            }
        }
        int total;
        const int q = written + psl_wg_compact<PSL_LPROJ_BS>(emit, s_wave, &total);
        if (emit && q < A.qstride) {
            const size_t r = (size_t)p * A.qstride + q;
            A.q[r] = row;
            psl_copy_desc(A.qdesc + r * 32, A.mldesc ? A.mldesc + (base + i) * 32 : A.ldesc + (base + i) * 32);
            if (A.owner) A.owner[r] = i;
        }
        written += total;
    }
    if (tid == 0) A.nq[p] = written;
}

const float kNoScale[1] = {1.0f};   // the frame line forms read no scale table: one level of 1 for the builder

int launch_line_frustum(pslfe_ctx* ctx, int nframes, const LineFrustumArgs& A, const ProjParams& P) {
    {
        PSL_STAGE_BEGIN(ctx, "line.project_frustum");
        k_line_project_frustum<<<dim3(1, nframes), PSL_LPROJ_BS, 0, ctx->stream>>>(A, P);
        PSL_STAGE_END(ctx, "line.project_frustum");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int launch_line_last(pslfe_ctx* ctx, int npairs, const LineLastArgs& A, const ProjParams& P) {
    {
        PSL_STAGE_BEGIN(ctx, "line.project_last");
        k_line_project_last<<<dim3(1, npairs), PSL_LPROJ_BS, 0, ctx->stream>>>(A, P);
        PSL_STAGE_END(ctx, "line.project_last");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_line_project_frustum_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw, const PslMapLineGeom* d_ml, const uint8_t* d_mldesc,
                                      const int32_t* d_nml, int mlstride, const PslCamera* cam, float log_scale_factor, float view_cos_limit,
                                      float th, float min_x, float min_y, float max_x, float max_y, PslLineQuery* d_queries, uint8_t* d_qdesc,
                                      int32_t* d_owner, int32_t* d_nq, int qstride, uint8_t* d_inview, int32_t* d_level, float* d_viewcos) {
    static const char* what = "pslfe_line_project_frustum_device";
    PSL_REQUIRE(ctx && d_Tcw && d_ml && d_mldesc && d_nml && d_queries && d_qdesc && d_nq, PSLFE_E_INVALID, "%s: NULL argument", what);
    PSL_REQUIRE(nframes >= 1 && mlstride >= 1 && qstride >= 1, PSLFE_E_INVALID, "%s: nframes %d mlstride %d qstride %d", what, nframes,
                mlstride, qstride);
    PSL_REQUIRE(cam, PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, kNoScale, 1, log_scale_factor, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    P.view_cos_limit = view_cos_limit;
    LineFrustumArgs A = {d_Tcw, d_ml, d_mldesc, d_nml, mlstride, d_queries, d_qdesc, d_owner, d_nq, qstride, d_inview, d_level, d_viewcos};
    PSL_HIP(hipSetDevice(ctx->device));
    return launch_line_frustum(ctx, nframes, A, P);
}

int pslfe_line_project_frustum(pslfe_ctx* ctx, const PslPose* Tcw, const PslMapLineGeom* ml, const uint8_t* mldesc, int nml, const PslCamera* cam,
                               float log_scale_factor, float view_cos_limit, float th, float min_x, float min_y, float max_x, float max_y,
                               PslLineQuery* queries, uint8_t* qdesc, int32_t* owner, int* nq, int qcap, uint8_t* inview, int32_t* level,
                               float* viewcos) {
    static const char* what = "pslfe_line_project_frustum";
    PSL_REQUIRE(ctx && Tcw && nq && nml >= 0 && qcap >= 0 && (nml == 0 || (ml && mldesc)) && (qcap == 0 || (queries && qdesc)) && cam,
                PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, kNoScale, 1, log_scale_factor, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    P.view_cos_limit = view_cos_limit;
    *nq = 0;
    if (nml == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    rc = psl_scratch_begin(ctx);
    if (rc) return rc;
    const size_t M = (size_t)nml;
    hipError_t e = hipSuccess;
    LineFrustumArgs A;
    A.Tcw = psl_scratch_up(ctx, Tcw, 1, st, &e);
    A.ml = psl_scratch_up(ctx, ml, M, st, &e);
    A.mldesc = psl_scratch_up(ctx, mldesc, M * 32, st, &e);
    A.nml = psl_scratch_up(ctx, &nml, 1, st, &e);
    A.mlstride = nml;
    A.q = psl_scratch_up<PslLineQuery>(ctx, nullptr, M, st, &e);
    A.qdesc = psl_scratch_up<uint8_t>(ctx, nullptr, M * 32, st, &e);
    A.owner = psl_scratch_up<int32_t>(ctx, nullptr, M, st, &e);
    A.nq = psl_scratch_up<int32_t>(ctx, nullptr, 1, st, &e);
    A.qstride = nml;
    A.inview = psl_scratch_up<uint8_t>(ctx, nullptr, M, st, &e);
    A.level = psl_scratch_up<int32_t>(ctx, nullptr, M, st, &e);
    A.viewcos = psl_scratch_up<float>(ctx, nullptr, M, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", what, hipGetErrorString(e));
    rc = launch_line_frustum(ctx, 1, A, P);
    if (rc) return rc;
    if (inview) PSL_HIP(hipMemcpyAsync(inview, A.inview, M, hipMemcpyDeviceToHost, st));
    if (level) PSL_HIP(hipMemcpyAsync(level, A.level, M * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (viewcos) PSL_HIP(hipMemcpyAsync(viewcos, A.viewcos, M * sizeof(float), hipMemcpyDeviceToHost, st));
    return psl_fetch_rows(ctx, A.nq, A.q, A.qdesc, A.owner, queries, qdesc, owner, nq, qcap, what, "lines in view");
}

int pslfe_line_project_last_device(pslfe_ctx* ctx, int npairs, const PslKeyLine* d_kls_last, const uint8_t* d_ldesc_last,
                                   const int32_t* d_nkl_last, int kl_stride, const PslLastLine* d_lines, const uint8_t* d_mldesc,
                                   const PslPose* d_Tcw, const PslCamera* cam, float th, float min_x, float min_y, float max_x, float max_y,
                                   PslLineQuery* d_queries, uint8_t* d_qdesc, int32_t* d_owner, int32_t* d_nq, int qstride) {
    static const char* what = "pslfe_line_project_last_device";
    PSL_REQUIRE(ctx && d_kls_last && d_ldesc_last && d_nkl_last && d_lines && d_Tcw && d_queries && d_qdesc && d_nq, PSLFE_E_INVALID,
                "%s: NULL argument", what);
    PSL_REQUIRE(npairs >= 1 && kl_stride >= 1 && qstride >= 1, PSLFE_E_INVALID, "%s: npairs %d kl_stride %d qstride %d", what, npairs,
                kl_stride, qstride);
    PSL_REQUIRE(cam, PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, kNoScale, 1, 0.f, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    LineLastArgs A = {d_kls_last, d_ldesc_last, d_nkl_last, kl_stride, d_lines, d_mldesc, d_Tcw, d_queries, d_qdesc, d_owner, d_nq, qstride};
    PSL_HIP(hipSetDevice(ctx->device));
    return launch_line_last(ctx, npairs, A, P);
}

int pslfe_line_project_last(pslfe_ctx* ctx, const PslKeyLine* kls_last, const uint8_t* ldesc_last, int n, const PslLastLine* lines,
                            const uint8_t* mldesc, const PslPose* Tcw, const PslCamera* cam, float th, float min_x, float min_y, float max_x,
                            float max_y, PslLineQuery* queries, uint8_t* qdesc, int32_t* owner, int* nq, int qcap) {
    static const char* what = "pslfe_line_project_last";
    PSL_REQUIRE(ctx && Tcw && nq && n >= 0 && qcap >= 0 && (n == 0 || (kls_last && ldesc_last && lines)) && (qcap == 0 || (queries && qdesc)) &&
                cam, PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, kNoScale, 1, 0.f, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    *nq = 0;
    if (n == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    rc = psl_scratch_begin(ctx);
    if (rc) return rc;
    const size_t N = (size_t)n;
    hipError_t e = hipSuccess;
    LineLastArgs A;
    A.kls = psl_scratch_up(ctx, kls_last, N, st, &e);
    A.ldesc = psl_scratch_up(ctx, ldesc_last, N * 32, st, &e);
    A.nkl = psl_scratch_up(ctx, &n, 1, st, &e);
    A.kl_stride = n;
    A.lines = psl_scratch_up(ctx, lines, N, st, &e);
    A.mldesc = mldesc ? psl_scratch_up(ctx, mldesc, N * 32, st, &e) : nullptr;
    A.Tcw = psl_scratch_up(ctx, Tcw, 1, st, &e);
    A.q = psl_scratch_up<PslLineQuery>(ctx, nullptr, N, st, &e);
    A.qdesc = psl_scratch_up<uint8_t>(ctx, nullptr, N * 32, st, &e);
    A.owner = psl_scratch_up<int32_t>(ctx, nullptr, N, st, &e);
    A.nq = psl_scratch_up<int32_t>(ctx, nullptr, 1, st, &e);
    A.qstride = n;
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", what, hipGetErrorString(e));
    rc = launch_line_last(ctx, 1, A, P);
    if (rc) return rc;
    return psl_fetch_rows(ctx, A.nq, A.q, A.qdesc, A.owner, queries, qdesc, owner, nq, qcap, what, "lines in view");
}

}  // extern "C"
