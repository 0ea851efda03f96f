// libpslfe: projection of map points into keyframes, in front of the KeyFrame-rate window searches of pslfe_kf.hip and
// pslfe_loop.hip.  Product code.
// Reference behaviour reproduced (all per-point arithmetic up to GetFeaturesInArea):
//   ORBmatcher::Fuse(pKF, vpMapPoints, th)                         src/ORBmatcher.cc:842-890      (PSLFE_KF_PROJ_FUSE)
//   ORBmatcher::Fuse(pKF, Scw, vpPoints, th, vpReplacePoint)       src/ORBmatcher.cc:1000-1050    (PSLFE_KF_PROJ_SCW)
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, ...)        src/ORBmatcher.cc:312-360      (PSLFE_KF_PROJ_SCW)
//   ORBmatcher::SearchBySim3, one direction                         src/ORBmatcher.cc:1148-1189, 1228-1269 (PSLFE_KF_PROJ_SIM3)
//   KeyFrame::IsInImage                                             src/KeyFrame.cc:726-729
//   MapPoint::PredictScale(dist, KeyFrame*)                         src/MapPoint.cc:385-400
// Conventions: include/pslfe.h above PslPose and above PslKfView; helpers: proj_kernels.h; differences from the frame forms: DESIGN.md §5.0h.
//
// K keyframes x M map points, one thread per pair (keyframes on blockIdx.y).  Rows are not compacted - the searches index by map
// point - so there is no scan: a thread reads 32 B of geometry and one skip byte and writes 32 B.  k_kf_centres gives every
// keyframe its camera centre once; a workgroup stages its keyframe's view and centre in LDS.
#include <stddef.h>
#include <string.h>

#include "pslfe_internal.h"
#include "psl_device_math.h"

#include "match_kernels.h"
#include "proj_kernels.h"
#include "kf_project.h"

#define PSL_KFP_BS 256
#define PSL_KFP_VIEW_WORDS (sizeof(PslKfView) / 4)

static_assert(offsetof(PslKfView, Tcw) == 0 && sizeof(PslKfView) == 100 && sizeof(PslMapPointGeom) == 32 && sizeof(PslProjQuery) == 32, "keyframe projection PODs");

// Ow = -Rcw.t()*tcw of every pose (KeyFrame::SetPose src/KeyFrame.cc:132-145; src/ORBmatcher.cc:303, :988 for a decomposed Scw;
// KeyFrame::GetCameraCenter for the line Fuse, which also starts from stop[k] = M)
__global__ __launch_bounds__(64) void k_kf_centres(const uint8_t* __restrict__ poses, int stride, int K, float* __restrict__ ow,
                                                   int32_t* __restrict__ stop, int M) {
    const int k = blockIdx.x * 64 + threadIdx.x;
    if (k >= K) return;
    float c[3];
    psl_centre(*reinterpret_cast<const PslPose*>(poses + (size_t)k * stride), c);
    ow[3 * k] = c[0]; ow[3 * k + 1] = c[1]; ow[3 * k + 2] = c[2];
    if (stop) stop[k] = M;
}

void psl_proj_centres_launch(hipStream_t st, const void* d_poses, int stride, int K, float* d_ow, int32_t* d_stop, int M) {
    k_kf_centres<<<(K + 63) / 64, 64, 0, st>>>(static_cast<const uint8_t*>(d_poses), stride, K, d_ow, d_stop, M);
}

struct KfProjArgs {
    const PslKfView* views;
    const float* ow;   // [K][3]; NULL in mode 2
    const float4* mp;  // PslMapPointGeom rows as two 16-byte halves
    const uint8_t* skip;
    int M;
    uint4* q;          // PslProjQuery rows as two 16-byte halves
    int32_t* level;
};

template <int MODE>
__global__ __launch_bounds__(PSL_KFP_BS) void k_kf_project(KfProjArgs A, ProjParams P) {
    __shared__ float s_view[PSL_KFP_VIEW_WORDS + 3];
    const int k = blockIdx.y, tid = threadIdx.x;
    if (tid < (int)PSL_KFP_VIEW_WORDS) s_view[tid] = reinterpret_cast<const float*>(A.views + k)[tid];
    else if (tid < (int)PSL_KFP_VIEW_WORDS + 3) s_view[tid] = MODE == PSLFE_KF_PROJ_SIM3 ? 0.f : A.ow[3 * k + tid - (int)PSL_KFP_VIEW_WORDS];
    __syncthreads();
    const int i = blockIdx.x * PSL_KFP_BS + tid;
    if (i >= A.M) return;
    const size_t row = (size_t)k * A.M + i;
    const float* R = s_view;        // Tcw.R
    const float* t = s_view + 9;    // Tcw.t
    const float* R2 = s_view + 12;  // T21.R
    const float* t2 = s_view + 21;  // T21.t
    const float* Ow = s_view + PSL_KFP_VIEW_WORDS;
    const PslCamera& C = P.cam;

    int lvl = -1;
    float u = 0.f, v = 0.f, ur = 0.f, radius = -1.0f;
    if (!(A.skip && A.skip[row])) {
        const float4 g0 = A.mp[2 * (size_t)i], g1 = A.mp[2 * (size_t)i + 1];  // x y z nx | ny nz min_dist max_dist
        float Xc[3];
        psl_pose_mul(R, t, g0.x, g0.y, g0.z, Xc);
        if (MODE == PSLFE_KF_PROJ_SIM3) psl_pose_mul(R2, t2, Xc[0], Xc[1], Xc[2], Xc);  // p3Dc2 = sR21*p3Dc1 + t21 (:1160)
        const float X = Xc[0], Y = Xc[1], Z = Xc[2];
        if (Z > 0.f) {
            // `1/p3Dc.at<float>(2)` (:859) is a float division, `1.0/...` (:1019, :1166) a double one rounded to float
            const float invz = MODE == PSLFE_KF_PROJ_FUSE ? PSL_FDIV(1.0f, Z) : (float)PSL_DDIV(1.0, (double)Z);
            const float x = PSL_FMUL(X, invz), y = PSL_FMUL(Y, invz);
            const float pu = PSL_FADD(PSL_FMUL(C.fx, x), C.cx), pv = PSL_FADD(PSL_FMUL(C.fy, y), C.cy);
            if (pu >= P.minX && pu < P.maxX && pv >= P.minY && pv < P.maxY) {  // KeyFrame::IsInImage
                const float maxD = PSL_FMUL(1.2f, g1.w), minD = PSL_FMUL(0.8f, g1.z);
                float dist;
                bool ok;
                if (MODE == PSLFE_KF_PROJ_SIM3) {
                    dist = psl_norm3(X, Y, Z);  // cv::norm(p3Dc2) (:1179)
                    ok = !(dist < minD || dist > maxD);
                } else {
                    const float p0 = PSL_FSUB(g0.x, Ow[0]), p1 = PSL_FSUB(g0.y, Ow[1]), p2 = PSL_FSUB(g0.z, Ow[2]);  // PO = p3Dw - Ow
                    dist = psl_norm3(p0, p1, p2);
                    ok = !(dist < minD || dist > maxD);
                    // `PO.dot(Pn) < 0.5*dist3D` (:884): a double compare
                    ok = ok && !(psl_dot3(p0, p1, p2, g0.w, g1.x, g1.y) < PSL_DMUL(0.5, (double)dist));
                }
                if (ok) {
                    lvl = psl_predict_level(g1.w, dist, P.log_scale_factor, P.nlevels);
                    u = pu;
                    v = pv;
                    ur = PSL_FSUB(pu, PSL_FMUL(C.bf, invz));
                    radius = PSL_FMUL(P.th, P.scale[lvl]);
                }
            }
        }
    }
    // min_level = level - 1, max_level = level; a dropped row is radius = -1 and zeros
    A.q[2 * row] = make_uint4(__float_as_uint(u), __float_as_uint(v), __float_as_uint(radius), __float_as_uint(ur));
    A.q[2 * row + 1] = make_uint4(lvl >= 0 ? (uint32_t)(lvl - 1) : 0u, lvl >= 0 ? (uint32_t)lvl : 0u, 0u, 0u);
    if (A.level) A.level[row] = lvl;
}

int psl_proj_params(ProjParams* P, int mode, const PslCamera* cam, float min_x, float min_y, float max_x, float max_y,
                    const float* scale_factors, int nlevels, float log_scale_factor, float th, const char* who) {
    PSL_REQUIRE(cam && scale_factors, PSLFE_E_INVALID, "%s: NULL camera or scale factors", who);
    PSL_REQUIRE(nlevels >= 1 && nlevels <= PSLFE_MAX_LEVELS, PSLFE_E_INVALID, "%s: nlevels %d (1..%d)", who, nlevels, PSLFE_MAX_LEVELS);
    memset(P, 0, sizeof(*P));
    P->cam = *cam;
    memcpy(P->scale, scale_factors, (size_t)nlevels * sizeof(float));
    P->nlevels = nlevels;
    P->mode = mode;
    P->th = th;
    P->log_scale_factor = log_scale_factor;
    P->minX = min_x; P->minY = min_y; P->maxX = max_x; P->maxY = max_y;
    return PSLFE_OK;
}

int psl_kf_project_launch(pslfe_ctx* ctx, const ProjParams& P, const PslKfView* d_views, int K, const PslMapPointGeom* d_mp,
                          const uint8_t* d_skip, int M, float* d_ow, PslProjQuery* d_q, int32_t* d_level) {
    hipStream_t st = ctx->stream;
    KfProjArgs A;
    A.views = d_views; A.ow = P.mode == PSLFE_KF_PROJ_SIM3 ? nullptr : d_ow; A.mp = reinterpret_cast<const float4*>(d_mp); A.skip = d_skip;
    A.M = M; A.q = reinterpret_cast<uint4*>(d_q); A.level = d_level;
    const dim3 grid((M + PSL_KFP_BS - 1) / PSL_KFP_BS, K);
    {
        PSL_STAGE_BEGIN(ctx, "kf.project");
        if (P.mode == PSLFE_KF_PROJ_SIM3) {
            k_kf_project<PSLFE_KF_PROJ_SIM3><<<grid, PSL_KFP_BS, 0, st>>>(A, P);
        } else {
            psl_proj_centres_launch(st, d_views, sizeof(PslKfView), K, d_ow, nullptr, 0);
            if (P.mode == PSLFE_KF_PROJ_FUSE) k_kf_project<PSLFE_KF_PROJ_FUSE><<<grid, PSL_KFP_BS, 0, st>>>(A, P);
            else k_kf_project<PSLFE_KF_PROJ_SCW><<<grid, PSL_KFP_BS, 0, st>>>(A, P);
        }
        PSL_STAGE_END(ctx, "kf.project");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int psl_kf_project_upload(pslfe_ctx* ctx, const ProjParams& P, const PslKfView* views, int K, const PslMapPointGeom* mp, const uint8_t* skip,
                          int M, bool want_level, KfProjBuffers* B, const char* who) {
    hipStream_t st = ctx->stream;
    const size_t rows = (size_t)K * M;
    hipError_t e = hipSuccess;
    B->views = psl_scratch_up(ctx, views, K, st, &e);
    B->mp = psl_scratch_up(ctx, mp, M, st, &e);
    B->skip = skip ? psl_scratch_up(ctx, skip, rows, st, &e) : nullptr;
    B->ow = psl_scratch_up<float>(ctx, nullptr, (size_t)K * 3, st, &e);
    B->q = psl_scratch_up<PslProjQuery>(ctx, nullptr, rows, st, &e);
    B->level = want_level ? psl_scratch_up<int32_t>(ctx, nullptr, rows, st, &e) : nullptr;
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    return psl_kf_project_launch(ctx, P, B->views, K, B->mp, B->skip, M, B->ow, B->q, B->level);
}

extern "C" {

int pslfe_kf_project(pslfe_kf* k, int mode, const PslKfView* views, int K, const PslMapPointGeom* mp, const uint8_t* skip, int M,
                     const PslCamera* cam, float min_x, float min_y, float max_x, float max_y, const float* scale_factors, int nlevels,
                     float log_scale_factor, float th, PslProjQuery* queries, int32_t* level) {
    static const char* who = "pslfe_kf_project";
    PSL_REQUIRE(k, PSLFE_E_INVALID, "%s: NULL handle", who);
    PSL_REQUIRE(K >= 0 && M >= 0, PSLFE_E_INVALID, "%s: K = %d, M = %d", who, K, M);
    PSL_REQUIRE(mode >= PSLFE_KF_PROJ_FUSE && mode <= PSLFE_KF_PROJ_SIM3, PSLFE_E_INVALID, "%s: mode %d (0..2)", who, mode);
    ProjParams P;
    if (int rc = psl_proj_params(&P, mode, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, log_scale_factor, th, who)) return rc;
    if (K == 0 || M == 0) return PSLFE_OK;
    PSL_REQUIRE(views && mp && queries, PSLFE_E_INVALID, "%s: NULL views, map points or output", who);
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    const size_t rows = (size_t)K * M;
    KfProjBuffers B;
    if (int rc = psl_kf_project_upload(ctx, P, views, K, mp, skip, M, level != nullptr, &B, who)) return rc;
    PSL_HIP(hipMemcpyAsync(queries, B.q, rows * sizeof(PslProjQuery), hipMemcpyDeviceToHost, st));
    if (level) PSL_HIP(hipMemcpyAsync(level, B.level, rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

}  // extern "C"
