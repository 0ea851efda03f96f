// Host side of the projections: the one params struct and its builder, the tail of the host-form entry points, the camera-centre
// launch, and the keyframe projection of pslfe_kf_project.hip as the searches of pslfe_kf.hip and pslfe_loop.hip chain it in front of
// their own kernels.  Product code.
#ifndef PSL_KF_PROJECT_H
#define PSL_KF_PROJECT_H

#include "pslfe_internal.h"

struct ProjParams {   // what every projection kernel takes by value; a form leaves what it does not read at zero
    PslCamera cam;
    float scale[PSLFE_MAX_LEVELS];
    int nlevels;
    float th, th_depth, log_scale_factor, view_cos_limit;   // th_depth, view_cos_limit, mono: frame forms
    int mono;
    float minX, minY, maxX, maxY;
    int mode;                                               // PSLFE_KF_PROJ_* (pslfe_kf_project.hip)
};
#define PSL_PROJ_NO_MODE (-1)           // every form but the keyframe point projection

struct KfProjBuffers {   // device, from the context's scratch arena
    const PslKfView* views;
    const PslMapPointGeom* mp;
    const uint8_t* skip;   // NULL: none
    float* ow;
    PslProjQuery* q;       // [K][M]
    int32_t* level;        // [K][M] or NULL
};

// checks cam, scale_factors and nlevels (1..PSLFE_MAX_LEVELS): PSLFE_E_INVALID with the text set.  What only some forms check stays
// with them: the mode (pslfe_kf_project), empty bounds and their own NULL text (the frame forms).  A form without a scale table passes
// one level of 1.
int psl_proj_params(ProjParams* P, int mode, const PslCamera* cam, float min_x, float min_y, float max_x, float max_y,
                    const float* scale_factors, int nlevels, float log_scale_factor, float th, const char* who);
// ow[3k..] = the camera centre of pose k (poses: K records of `stride` bytes that begin with a PslPose); stop != NULL: stop[k] = M
void psl_proj_centres_launch(hipStream_t st, const void* d_poses, int stride, int K, float* d_ow, int32_t* d_stop, int M);
// rows k*M + i of d_q (and d_level, may be NULL) on the context's stream; d_ow: K*3 floats of scratch
int psl_kf_project_launch(pslfe_ctx* ctx, const ProjParams& P, const PslKfView* d_views, int K, const PslMapPointGeom* d_mp,
                          const uint8_t* d_skip, int M, float* d_ow, PslProjQuery* d_q, int32_t* d_level);
// after psl_scratch_begin: uploads views, mp and skip (may be NULL), takes the outputs from the arena and launches
int psl_kf_project_upload(pslfe_ctx* ctx, const ProjParams& P, const PslKfView* views, int K, const PslMapPointGeom* mp, const uint8_t* skip,
                          int M, bool want_level, KfProjBuffers* B, const char* who);

// rows of a host-form call: the count, then (when it fits) the rows, descriptors and owners; noun: what the capacity error counts
template <typename Row>
int psl_fetch_rows(pslfe_ctx* ctx, const int32_t* dnq, const Row* dq, const uint8_t* dqd, const int32_t* dow, Row* queries, uint8_t* qdesc,
                   int32_t* owner, int* nq, int qcap, const char* what, const char* noun) {
    hipStream_t st = ctx->stream;
    int cnt = 0;
    PSL_HIP(hipMemcpyAsync(&cnt, dnq, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *nq = cnt;
    PSL_REQUIRE(cnt <= qcap, PSLFE_E_CAPACITY, "%s: %d %s, capacity %d", what, cnt, noun, qcap);
    if (cnt > 0) {
        PSL_HIP(hipMemcpyAsync(queries, dq, (size_t)cnt * sizeof(Row), hipMemcpyDeviceToHost, st));
        PSL_HIP(hipMemcpyAsync(qdesc, dqd, (size_t)cnt * 32, hipMemcpyDeviceToHost, st));
        if (owner) PSL_HIP(hipMemcpyAsync(owner, dow, (size_t)cnt * sizeof(int32_t), hipMemcpyDeviceToHost, st));
        PSL_HIP(hipStreamSynchronize(st));
    }
    return PSLFE_OK;
}

#endif
