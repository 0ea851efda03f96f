// The keyframe projection of pslfe_kf_project.hip as the searches of pslfe_kf.hip and pslfe_loop.hip chain it in front of their own
// kernels (host side).  Product code.
#ifndef PSL_KF_PROJECT_H
#define PSL_KF_PROJECT_H

#include "pslfe_internal.h"

struct KfProjParams {
    PslCamera cam;
    float scale[PSLFE_MAX_LEVELS];
    int nlevels, mode;
    float th, log_scale_factor;
    float minX, minY, maxX, maxY;
};

struct KfProjBuffers {   // device, from the context's scratch arena
    const PslKfView* views;
    const PslMapPointGeom* mp;
    const uint8_t* skip;   // NULL: none
    float* ow;
    PslProjQuery* q;       // [K][M]
    int32_t* level;        // [K][M] or NULL
};

// checks mode (0..2), cam, scale_factors and nlevels (1..PSLFE_MAX_LEVELS): PSLFE_E_INVALID with the text set
int psl_kf_proj_params(KfProjParams* P, int mode, const PslCamera* cam, float min_x, float min_y, float max_x, float max_y,
                       const float* scale_factors, int nlevels, float log_scale_factor, float th, const char* who);
// rows k*M + i of d_q (and d_level, may be NULL) on the context's stream; d_ow: K*3 floats of scratch
int psl_kf_project_launch(pslfe_ctx* ctx, const KfProjParams& P, const PslKfView* d_views, int K, const PslMapPointGeom* d_mp,
                          const uint8_t* d_skip, int M, float* d_ow, PslProjQuery* d_q, int32_t* d_level);
// after psl_scratch_begin: uploads views, mp and skip (may be NULL), takes the outputs from the arena and launches
int psl_kf_project_upload(pslfe_ctx* ctx, const KfProjParams& P, const PslKfView* views, int K, const PslMapPointGeom* mp, const uint8_t* skip,
                          int M, bool want_level, KfProjBuffers* B, const char* who);

#endif
