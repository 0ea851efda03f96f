// libpslfe: projection of 3-D points into a frame, up to the window searches of pslfe_match.hip.  Product code.
// Reference behaviour reproduced:
//   ORBmatcher::SearchByProjection(cur,last) up to GetFeaturesInArea     src/ORBmatcher.cc:1338-1390
//   Tracking::UpdateLastFrame "visual odometry" points (localisation)     src/Tracking.cc:1052-1104
//   Frame::UnprojectStereo                                               src/Frame.cc:1365-1379
//   Frame::isInFrustum + MapPoint::PredictScale                          src/Frame.cc:927-983, src/MapPoint.cc:402-416
//   ORBmatcher::SearchByProjection(F,MPs) up to GetFeaturesInArea        src/ORBmatcher.cc:45-70, RadiusByViewingCos :131-137
//
// cv::Mat arithmetic is not in the reference tree; its conventions are include/pslfe.h and DESIGN.md §3, the helpers proj_kernels.h,
// and what these frame forms do differently from the keyframe forms is the table of DESIGN.md §5.0h.
//
// One workgroup per frame (frames on blockIdx.y): thread t handles points t, t + 1024, ... and the emitted rows are compacted
// in point order by a workgroup scan, so the matchers' first-come-first-served order is the reference's loop order.
#include <string.h>

#include <vector>

#include "pslfe_internal.h"
#include "psl_device_math.h"

#include "match_kernels.h"
#include "proj_kernels.h"
#include "kf_project.h"

#define PSL_PROJ_BS 1024

namespace {

// UpdateLastFrame's selection (src/Tracking.cc:1065-1103): over the keypoints with mvDepth > 0 sorted by (z, i), the loop
// visits the first L = min(n_valid, max(n_close + 1, 101)) (n_close = #{z <= th_depth}; the break follows the increment).
// Returns the largest selected key ((float bits of z) << 12 | i), 0 when nothing is selected: keypoint i is selected iff
// its key is valid and <= the returned one.  LDS radix select, 8-bit digits over the 43 bits of a key.
__device__ uint64_t psl_vo_threshold(const float* __restrict__ depth, int n, float th_depth, uint64_t* s_key, int* s_hist, int* s_misc) {
    const int tid = threadIdx.x;
    if (tid < 2) s_misc[tid] = 0;
    __syncthreads();
    int nv = 0, nc = 0;
    for (int i = tid; i < n; i += PSL_PROJ_BS) {
        const float z = depth[i];
        const bool valid = z > 0.f;
        s_key[i] = valid ? ((uint64_t)__float_as_uint(z) << 12) | (uint64_t)i : ~0ull;
        nv += valid;
        nc += valid && z <= th_depth;
    }
    if (nv) atomicAdd(&s_misc[0], nv);
    if (nc) atomicAdd(&s_misc[1], nc);
    __syncthreads();
    const int n_valid = s_misc[0], n_close = s_misc[1];
    const int want = n_close + 1 > 101 ? n_close + 1 : 101;
    const int L = n_valid < want ? n_valid : want;
    if (L == 0) return 0ull;
    if (L == n_valid) return ~0ull - 1;  // every valid key (a valid key is < 2^43)
    uint64_t prefix = 0;
    int k = L - 1;  // rank of the wanted key among the valid ones
    for (int shift = 40; shift >= 0; shift -= 8) {
        __syncthreads();
        if (tid < 256) s_hist[tid] = 0;
        __syncthreads();
        const uint64_t hi = prefix >> (shift + 8);
        for (int i = tid; i < n; i += PSL_PROJ_BS) {
            const uint64_t key = s_key[i];
            if (key != ~0ull && (key >> (shift + 8)) == hi) atomicAdd(&s_hist[(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid < 64) {  // wave 0: lane l owns bins 4l..4l+3
            const int c0 = s_hist[4 * tid], c1 = s_hist[4 * tid + 1], c2 = s_hist[4 * tid + 2], c3 = s_hist[4 * tid + 3];
            const int own = c0 + c1 + c2 + c3;
            int incl = own;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (tid >= o) incl += u; }
            const int excl = incl - own;
            if (excl <= k && k < incl) {
                int r = k - excl, d = 4 * tid;
                if (r >= c0) { r -= c0; ++d; if (r >= c1) { r -= c1; ++d; if (r >= c2) { r -= c2; ++d; } } }
                s_misc[2] = d;
                s_misc[3] = r;
            }
        }
        __syncthreads();
        prefix |= (uint64_t)s_misc[2] << shift;
        k = s_misc[3];
    }
    return prefix;
}

struct LastArgs {
    FrameStore S;
    const float* depth;  // mvDepth [max_frames][cap]
    int slot0;
    const PslPose* Tlw;
    const PslPose* Tcw;
    const PslLastPoint* pts;  // [npairs][cap] or NULL
    const uint8_t* mpdesc;    // [npairs][cap][32] or NULL
    PslProjQuery* q;
    uint8_t* qdesc;
    int32_t* owner;
    int32_t* nq;
    int qstride;
};

template <bool VO>
__global__ __launch_bounds__(PSL_PROJ_BS) void k_project_last(LastArgs A, ProjParams P) {
    __shared__ uint64_t s_key[VO ? PSL_QMAX : 1];
    __shared__ int s_hist[256];
    __shared__ int s_misc[4];
    __shared__ int s_wave[PSL_PROJ_BS / 64];
    const int pair = blockIdx.y, slot = A.slot0 + pair, tid = threadIdx.x;
    const size_t base = (size_t)slot * A.S.cap, pbase = (size_t)pair * A.S.cap;
    const int n = min(A.S.meta[slot].n, A.S.cap);
    const float* depth = A.depth + base;
    const PslPose Tl = A.Tlw[pair], Tc = A.Tcw[pair];
    const PslCamera& C = P.cam;

    // pose algebra of :1338-1350
    float twc[3], tlc[3];
    psl_centre(Tc, twc);
#pragma unroll
    for (int r = 0; r < 3; ++r) tlc[r] = psl_affine_row(Tl.R[3 * r], Tl.R[3 * r + 1], Tl.R[3 * r + 2], twc[0], twc[1], twc[2], Tl.t[r]);
    const float mb = PSL_FDIV(C.bf, C.fx);
    const bool fwd = tlc[2] > mb && !P.mono;
    const bool bwd = -tlc[2] > mb && !P.mono;

    uint64_t thr = 0;
    float Ow[3] = {0.f, 0.f, 0.f};
    if (VO) {
        thr = psl_vo_threshold(depth, n, P.th_depth, s_key, s_hist, s_misc);
        psl_centre(Tl, Ow);
    }
    const float invfx = PSL_FDIV(1.0f, C.fx), invfy = PSL_FDIV(1.0f, C.fy);

    int written = 0;
    for (int i0 = 0; i0 < n; i0 += PSL_PROJ_BS) {
        const int i = i0 + tid;
        bool emit = false;
        PslProjQuery row;
        const uint8_t* dsrc = nullptr;
        if (i < n) {
            const PslKeyPoint kp = A.S.kps[base + i];
            PslLastPoint pt = {0.f, 0.f, 0.f, 0};
            if (A.pts) pt = A.pts[pbase + i];
            const int state = pt.state & 7;
            bool have = state != 0;
            int blocks = state >= 2;
            dsrc = A.mpdesc ? A.mpdesc + (pbase + i) * 32 : A.S.desc + (base + i) * 32;
            float X = pt.x, Y = pt.y, Z = pt.z;
            if (VO && state < 2) {
                const float z = depth[i];
                const uint64_t key = ((uint64_t)__float_as_uint(z) << 12) | (uint64_t)i;
                if (z > 0.f && key <= thr) {  // a new MapPoint(UnprojectStereo(i), ..., &mLastFrame, i) (src/MapPoint.cc:66)
                    const float xc = PSL_FMUL(PSL_FMUL(PSL_FSUB(kp.x, C.cx), z), invfx);
                    const float yc = PSL_FMUL(PSL_FMUL(PSL_FSUB(kp.y, C.cy), z), invfy);
                    X = psl_affine_row(Tl.R[0], Tl.R[3], Tl.R[6], xc, yc, z, Ow[0]);
                    Y = psl_affine_row(Tl.R[1], Tl.R[4], Tl.R[7], xc, yc, z, Ow[1]);
                    Z = psl_affine_row(Tl.R[2], Tl.R[5], Tl.R[8], xc, yc, z, Ow[2]);
                    have = true;
                    blocks = 0;
                    dsrc = A.S.desc + (base + i) * 32;
                }
            }
            if (have && !(pt.state & 8)) {
                const float xc = psl_affine_row(Tc.R[0], Tc.R[1], Tc.R[2], X, Y, Z, Tc.t[0]);
                const float yc = psl_affine_row(Tc.R[3], Tc.R[4], Tc.R[5], X, Y, Z, Tc.t[1]);
                const float zc = psl_affine_row(Tc.R[6], Tc.R[7], Tc.R[8], X, Y, Z, Tc.t[2]);
                if (zc > 0.f) {
                    const float invzc = (float)PSL_DDIV(1.0, (double)zc);  // `1.0/x3Dc.at<float>(2)` (:1360)
                    const float u = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fx, xc), invzc), C.cx);
                    const float v = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fy, yc), invzc), C.cy);
                    if (u >= P.minX && u <= P.maxX && v >= P.minY && v <= P.maxY) {
                        const int o = kp.octave;
                        const int oc = o < 0 ? 0 : (o >= P.nlevels ? P.nlevels - 1 : o);
                        row.u = u;
                        row.v = v;
                        row.radius = PSL_FMUL(P.th, P.scale[oc]);
                        row.ur = PSL_FSUB(u, PSL_FMUL(C.bf, invzc));
                        row.min_level = fwd ? o : (bwd ? 0 : o - 1);
                        row.max_level = fwd ? -1 : (bwd ? o : o + 1);
                        row.angle = kp.angle;
                        row.blocks = blocks;
                        emit = true;
                    }
                }
            }
        }
        int total;
        const int q = written + psl_wg_compact<PSL_PROJ_BS>(emit, s_wave, &total);
        if (emit && q < A.qstride) {
            const size_t r = (size_t)pair * A.qstride + q;
            A.q[r] = row;
            psl_copy_desc(A.qdesc + r * 32, dsrc);
            if (A.owner) A.owner[r] = i;
        }
        written += total;
    }
    if (tid == 0) A.nq[pair] = written;
}

struct FrustumArgs {
    const PslPose* Tcw;
    const PslMapPointGeom* mp;
    const uint8_t* mpdesc;
    const int32_t* nmp;
    int mpstride;
    PslProjQuery* q;
    uint8_t* qdesc;
    int32_t* owner;
    int32_t* nq;
    int qstride;
    uint8_t* inview;
    int32_t* level;
    float* viewcos;
};

__global__ __launch_bounds__(PSL_PROJ_BS) void k_project_frustum(FrustumArgs A, ProjParams P) {
    __shared__ int s_wave[PSL_PROJ_BS / 64];
    const int f = blockIdx.y, tid = threadIdx.x;
    const size_t base = (size_t)f * A.mpstride;
    const int n = min(A.nmp[f], A.mpstride);
    const PslPose T = A.Tcw[f];
    const PslCamera& C = P.cam;
    float Ow[3];
    psl_centre(T, Ow);
    int written = 0;
    for (int j0 = 0; j0 < n; j0 += PSL_PROJ_BS) {
        const int j = j0 + tid;
        bool emit = false;
        PslProjQuery row;
        int lvl = -1;
        float vc = 0.f;
        if (j < n) {
            const PslMapPointGeom G = A.mp[base + j];
            float Xc[3];
            psl_pose_mul(T.R, T.t, G.x, G.y, G.z, Xc);
            const float X = Xc[0], Y = Xc[1], Z = Xc[2];
            if (Z > 0.f) {
                const float invz = PSL_FDIV(1.0f, Z);
                const float u = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fx, X), invz), C.cx);
                const float v = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fy, Y), invz), C.cy);
                if (u >= P.minX && u <= P.maxX && v >= P.minY && v <= P.maxY) {
                    const float maxD = PSL_FMUL(1.2f, G.max_dist), minD = PSL_FMUL(0.8f, G.min_dist);
                    const float p0 = PSL_FSUB(G.x, Ow[0]), p1 = PSL_FSUB(G.y, Ow[1]), p2 = PSL_FSUB(G.z, Ow[2]);
                    const float dist = psl_norm3(p0, p1, p2);
                    if (!(dist < minD || dist > maxD)) {
                        const double dot = psl_dot3(p0, p1, p2, G.nx, G.ny, G.nz);
                        const float viewCos = (float)PSL_DDIV(dot, (double)dist);
                        if (!(viewCos < P.view_cos_limit)) {
                            lvl = psl_predict_level(G.max_dist, dist, P.log_scale_factor, P.nlevels);
                            vc = viewCos;
                            float r = (double)viewCos > 0.998 ? 2.5f : 4.0f;
                            if (P.th != 1.0f) r = PSL_FMUL(r, P.th);
                            row.u = u;
                            row.v = v;
                            row.radius = PSL_FMUL(r, P.scale[lvl]);
                            row.ur = PSL_FSUB(u, PSL_FMUL(C.bf, invz));
                            row.min_level = lvl - 1;
                            row.max_level = lvl;
                            row.angle = 0.f;
                            row.blocks = 1;
                            emit = true;
                        }
                    }
                }
            }
            if (A.inview) A.inview[base + j] = emit ? 1 : 0;
            if (A.level) A.level[base + j] = lvl;
            if (A.viewcos) A.viewcos[base + j] = vc;
        }
        int total;
        const int q = written + psl_wg_compact<PSL_PROJ_BS>(emit, s_wave, &total);
        if (emit && q < A.qstride) {
            const size_t r = (size_t)f * A.qstride + q;
            A.q[r] = row;
            psl_copy_desc(A.qdesc + r * 32, A.mpdesc + (base + j) * 32);
            if (A.owner) A.owner[r] = j;
        }
        written += total;
    }
    if (tid == 0) A.nq[f] = written;
}

int launch_project_last(pslfe_frame* last, int slot0, int npairs, const PslPose* d_Tlw, const PslPose* d_Tcw, const PslLastPoint* d_points,
                        const uint8_t* d_mpdesc, const ProjParams& P, int vo, PslProjQuery* d_queries, uint8_t* d_qdesc, int32_t* d_owner,
                        int32_t* d_nq, int qstride) {
    LastArgs A;
    A.S = last->S; A.depth = last->d_depth; A.slot0 = slot0; A.Tlw = d_Tlw; A.Tcw = d_Tcw; A.pts = d_points; A.mpdesc = d_mpdesc;
    A.q = d_queries; A.qdesc = d_qdesc; A.owner = d_owner; A.nq = d_nq; A.qstride = qstride;
    {
        PSL_STAGE_BEGIN(last->ctx, "project.last");
        if (vo) k_project_last<true><<<dim3(1, npairs), PSL_PROJ_BS, 0, last->ctx->stream>>>(A, P);
        else k_project_last<false><<<dim3(1, npairs), PSL_PROJ_BS, 0, last->ctx->stream>>>(A, P);
        PSL_STAGE_END(last->ctx, "project.last");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int check_last(pslfe_frame* last, int slot0, int npairs, int vo, float th_depth, int qstride, const char* what) {
    PSL_REQUIRE(npairs >= 1 && slot0 >= 0 && slot0 + npairs <= last->max_frames, PSLFE_E_INVALID, "%s: slots %d..%d of %d", what, slot0,
                slot0 + npairs - 1, last->max_frames);
    PSL_REQUIRE(qstride >= 1, PSLFE_E_INVALID, "%s: qstride %d", what, qstride);
    PSL_REQUIRE(qstride <= last->cap, PSLFE_E_CAPACITY, "%s: qstride %d > capacity %d", what, qstride, last->cap);
    PSL_REQUIRE(th_depth == th_depth, PSLFE_E_INVALID, "%s: th_depth is NaN", what);
    for (int s = slot0; s < slot0 + npairs; ++s) {
        PSL_REQUIRE(last->slot_set[s], PSLFE_E_STATE, "%s: slot %d not set", what, s);
        PSL_REQUIRE(!vo || last->slot_depth[s], PSLFE_E_STATE, "%s: visual-odometry points need depth, slot %d has none", what, s);
    }
    return PSLFE_OK;
}

int launch_project_frustum(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw, const PslMapPointGeom* d_mp, const uint8_t* d_mpdesc,
                           const int32_t* d_nmp, int mpstride, const ProjParams& P, PslProjQuery* d_queries, uint8_t* d_qdesc,
                           int32_t* d_owner, int32_t* d_nq, int qstride, uint8_t* d_inview, int32_t* d_level, float* d_viewcos) {
    FrustumArgs A;
    A.Tcw = d_Tcw; A.mp = d_mp; A.mpdesc = d_mpdesc; A.nmp = d_nmp; A.mpstride = mpstride; A.q = d_queries; A.qdesc = d_qdesc;
    A.owner = d_owner; A.nq = d_nq; A.qstride = qstride; A.inview = d_inview; A.level = d_level; A.viewcos = d_viewcos;
    {
        PSL_STAGE_BEGIN(ctx, "project.frustum");
        k_project_frustum<<<dim3(1, nframes), PSL_PROJ_BS, 0, ctx->stream>>>(A, P);
        PSL_STAGE_END(ctx, "project.frustum");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_orb_project_last_device(pslfe_frame* last, int last_slot0, int npairs, const PslPose* d_Tlw, const PslPose* d_Tcw,
                                  const PslLastPoint* d_points, const uint8_t* d_mpdesc, const PslCamera* cam, const float* scale_factors,
                                  int nlevels, float th, float th_depth, int mono, int vo, float min_x, float min_y, float max_x,
                                  float max_y, PslProjQuery* d_queries, uint8_t* d_qdesc, int32_t* d_owner, int32_t* d_nq, int qstride) {
    static const char* what = "pslfe_orb_project_last_device";
    PSL_REQUIRE(last && d_Tlw && d_Tcw && d_queries && d_qdesc && d_nq && cam && scale_factors, PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, 0.f, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    P.th_depth = th_depth; P.mono = mono;
    rc = check_last(last, last_slot0, npairs, vo, th_depth, qstride, what);
    if (rc) return rc;
    PSL_HIP(hipSetDevice(last->ctx->device));
    return launch_project_last(last, last_slot0, npairs, d_Tlw, d_Tcw, d_points, d_mpdesc, P, vo, d_queries, d_qdesc, d_owner, d_nq, qstride);
}

int pslfe_orb_project_last(pslfe_frame* last, int slot, const PslPose* Tlw, const PslPose* Tcw, const PslLastPoint* points,
                           const uint8_t* mpdesc, const PslCamera* cam, const float* scale_factors, int nlevels, float th, float th_depth,
                           int mono, int vo, float min_x, float min_y, float max_x, float max_y, PslProjQuery* queries, uint8_t* qdesc,
                           int32_t* owner, int* nq, int qcap) {
    static const char* what = "pslfe_orb_project_last";
    PSL_REQUIRE(last && Tlw && Tcw && nq && qcap >= 0 && (qcap == 0 || (queries && qdesc)) && cam && scale_factors, PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, 0.f, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    P.th_depth = th_depth; P.mono = mono;
    rc = check_last(last, slot, 1, vo, th_depth, last->cap, what);
    if (rc) return rc;
    *nq = 0;
    pslfe_ctx* ctx = last->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    FrameMeta m;
    PSL_HIP(hipMemcpyAsync(&m, last->S.meta + slot, sizeof(m), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    const size_t n = (size_t)(m.n < last->cap ? m.n : last->cap), K = (size_t)last->cap;
    rc = psl_scratch_begin(ctx);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    const PslPose* dTl = psl_scratch_up(ctx, Tlw, 1, st, &e);
    const PslPose* dTc = psl_scratch_up(ctx, Tcw, 1, st, &e);
    const PslLastPoint* dp = points ? psl_scratch_up(ctx, points, n, st, &e) : nullptr;
    const uint8_t* dd = mpdesc ? psl_scratch_up(ctx, mpdesc, n * 32, st, &e) : nullptr;
    PslProjQuery* dq = psl_scratch_up<PslProjQuery>(ctx, nullptr, K, st, &e);
    uint8_t* dqd = psl_scratch_up<uint8_t>(ctx, nullptr, K * 32, st, &e);
    int32_t* dow = psl_scratch_up<int32_t>(ctx, nullptr, K, st, &e);
    int32_t* dnq = psl_scratch_up<int32_t>(ctx, nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", what, hipGetErrorString(e));
    rc = launch_project_last(last, slot, 1, dTl, dTc, dp, dd, P, vo, dq, dqd, dow, dnq, (int)K);
    if (rc) return rc;
    return psl_fetch_rows(ctx, dnq, dq, dqd, dow, queries, qdesc, owner, nq, qcap, what, "rows");
}

int pslfe_orb_project_frustum_device(pslfe_ctx* ctx, int nframes, const PslPose* d_Tcw, const PslMapPointGeom* d_mp, const uint8_t* d_mpdesc,
                                     const int32_t* d_nmp, int mpstride, const PslCamera* cam, const float* scale_factors, int nlevels,
                                     float log_scale_factor, float view_cos_limit, float th, float min_x, float min_y, float max_x,
                                     float max_y, PslProjQuery* d_queries, uint8_t* d_qdesc, int32_t* d_owner, int32_t* d_nq, int qstride,
                                     uint8_t* d_inview, int32_t* d_level, float* d_viewcos) {
    static const char* what = "pslfe_orb_project_frustum_device";
    PSL_REQUIRE(ctx && d_Tcw && d_mp && d_mpdesc && d_nmp && d_queries && d_qdesc && d_nq, PSLFE_E_INVALID, "%s: NULL argument", what);
    PSL_REQUIRE(nframes >= 1 && mpstride >= 1 && qstride >= 1, PSLFE_E_INVALID, "%s: nframes %d mpstride %d qstride %d", what, nframes,
                mpstride, qstride);
    PSL_REQUIRE(cam && scale_factors, PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, log_scale_factor, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    P.view_cos_limit = view_cos_limit;
    PSL_HIP(hipSetDevice(ctx->device));
    return launch_project_frustum(ctx, nframes, d_Tcw, d_mp, d_mpdesc, d_nmp, mpstride, P, d_queries, d_qdesc, d_owner, d_nq, qstride,
                                  d_inview, d_level, d_viewcos);
}

int pslfe_orb_project_frustum(pslfe_ctx* ctx, const PslPose* Tcw, const PslMapPointGeom* mp, const uint8_t* mpdesc, int nmp,
                              const PslCamera* cam, const float* scale_factors, int nlevels, float log_scale_factor, float view_cos_limit,
                              float th, float min_x, float min_y, float max_x, float max_y, PslProjQuery* queries, uint8_t* qdesc,
                              int32_t* owner, int* nq, int qcap, uint8_t* inview, int32_t* level, float* viewcos) {
    static const char* what = "pslfe_orb_project_frustum";
    PSL_REQUIRE(ctx && Tcw && nq && nmp >= 0 && qcap >= 0 && (nmp == 0 || (mp && mpdesc)) && (qcap == 0 || (queries && qdesc)) && cam &&
                scale_factors, PSLFE_E_INVALID, "%s: NULL argument", what);
    ProjParams P;
    int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, log_scale_factor, th, what);
    if (rc) return rc;
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    P.view_cos_limit = view_cos_limit;
    *nq = 0;
    if (nmp == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    rc = psl_scratch_begin(ctx);
    if (rc) return rc;
    const size_t M = (size_t)nmp;
    hipError_t e = hipSuccess;
    const PslPose* dT = psl_scratch_up(ctx, Tcw, 1, st, &e);
    const PslMapPointGeom* dmp = psl_scratch_up(ctx, mp, M, st, &e);
    const uint8_t* dmd = psl_scratch_up(ctx, mpdesc, M * 32, st, &e);
    const int32_t* dn = psl_scratch_up(ctx, &nmp, 1, st, &e);
    PslProjQuery* dq = psl_scratch_up<PslProjQuery>(ctx, nullptr, M, st, &e);
    uint8_t* dqd = psl_scratch_up<uint8_t>(ctx, nullptr, M * 32, st, &e);
    int32_t* dow = psl_scratch_up<int32_t>(ctx, nullptr, M, st, &e);
    int32_t* dnq = psl_scratch_up<int32_t>(ctx, nullptr, 1, st, &e);
    uint8_t* div = psl_scratch_up<uint8_t>(ctx, nullptr, M, st, &e);
    int32_t* dlv = psl_scratch_up<int32_t>(ctx, nullptr, M, st, &e);
    float* dvc = psl_scratch_up<float>(ctx, nullptr, M, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", what, hipGetErrorString(e));
    rc = launch_project_frustum(ctx, 1, dT, dmp, dmd, dn, nmp, P, dq, dqd, dow, dnq, nmp, div, dlv, dvc);
    if (rc) return rc;
    if (inview) PSL_HIP(hipMemcpyAsync(inview, div, M, hipMemcpyDeviceToHost, st));
    if (level) PSL_HIP(hipMemcpyAsync(level, dlv, M * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (viewcos) PSL_HIP(hipMemcpyAsync(viewcos, dvc, M * sizeof(float), hipMemcpyDeviceToHost, st));
    return psl_fetch_rows(ctx, dnq, dq, dqd, dow, queries, qdesc, owner, nq, qcap, what, "map points in view");
}

}  // extern "C"
