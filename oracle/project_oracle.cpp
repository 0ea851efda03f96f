// Sequential C++ restatement of the projection entry points of include/pslfe.h (psl-slam_amd/csrc/pslfe_project.hip), written
// from the reference's loops (src/ORBmatcher.cc:45-70, 1338-1390; src/Frame.cc:927-983, 1365-1379; src/Tracking.cc:1052-1104;
// src/MapPoint.cc:402-416) and the arithmetic conventions stated in include/pslfe.h.  Test infrastructure: part of the oracle
// library; the tests compare the HIP kernels with it field by field.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../include/pslfe.h"
#define PSL_F64_QUAL static inline
#include "../psl-slam_amd/csrc/psl_f64math.h"
#include "psl_oracle.h"
#include "psl_oracle_internal.h"

using pso::affine;
// -R.t() * t
static void centre(const PslPose& T, float* c) { pso::centre(T.R, T.t, c); }

static int predict_level(float ratio, float log_scale_factor, int nlevels, int host_log) {
    if (!(ratio > 0.f)) return 0;
    if (isinf(ratio)) return nlevels - 1;
    const double l = host_log ? log((double)ratio) : psl_log((double)ratio);
    const double ls = ceil(l / (double)log_scale_factor);
    return ls > 0.0 ? (ls < (double)nlevels ? (int)ls : nlevels - 1) : 0;
}

extern "C" {

void pr_sizes(int32_t* out) {
    out[0] = (int32_t)sizeof(PslPose);
    out[1] = (int32_t)sizeof(PslLastPoint);
    out[2] = (int32_t)sizeof(PslMapPointGeom);
    out[3] = (int32_t)sizeof(PslProjQuery);
}

// UpdateLastFrame's selection as "sort by (z, i), keep the first L": sel[i] = 1 for the visited keypoints.
int pr_vo_select(const float* depth, int n, float th_depth, uint8_t* sel) {
    std::vector<std::pair<float, int>> v;
    int n_close = 0;
    for (int i = 0; i < n; ++i) {
        sel[i] = 0;
        if (depth[i] > 0) {
            v.push_back(std::make_pair(depth[i], i));
            n_close += depth[i] <= th_depth;
        }
    }
    std::sort(v.begin(), v.end());
    const int L = std::min((int)v.size(), std::max(n_close + 1, 101));
    for (int j = 0; j < L; ++j) sel[v[j].second] = 1;
    return L;
}

// Predicted levels of every float ratio in [lo, hi] with psl_log and with the host's log: the number of disagreements.
long pr_level_sweep(float lo, float hi, float log_scale_factor, int nlevels, long* nsamples) {
    long bad = 0, cnt = 0;
    for (float r = lo; r <= hi; r = nextafterf(r, INFINITY), ++cnt)
        bad += predict_level(r, log_scale_factor, nlevels, 0) != predict_level(r, log_scale_factor, nlevels, 1);
    *nsamples = cnt;
    return bad;
}

int pr_predict_level(float ratio, float log_scale_factor, int nlevels) { return predict_level(ratio, log_scale_factor, nlevels, 0); }

// kps / desc / depth: the last frame's mvKeysUn, descriptors, mvDepth (n entries); points / mpdesc may be NULL.
// bounds = {minX, minY, maxX, maxY}.  Returns the row count.
int pr_project_last(const PslKeyPoint* kps, const uint8_t* desc, const float* depth, int n, const PslPose* Tlw, const PslPose* Tcw,
                    const PslLastPoint* points, const uint8_t* mpdesc, const PslCamera* cam, const float* scale, int nlevels, float th,
                    float th_depth, int mono, int vo, const float* bounds, PslProjQuery* q, uint8_t* qdesc, int32_t* owner) {
    const PslCamera& C = *cam;
    const PslPose &Tl = *Tlw, &Tc = *Tcw;
    // LastFrame.mvpMapPoints after UpdateLastFrame
    std::vector<PslLastPoint> P(n);
    std::vector<const uint8_t*> D(n);
    std::vector<int> blocks(n);
    for (int i = 0; i < n; ++i) {
        P[i] = points ? points[i] : PslLastPoint{0.f, 0.f, 0.f, 0};
        D[i] = mpdesc ? mpdesc + (size_t)i * 32 : desc + (size_t)i * 32;
        blocks[i] = (P[i].state & 7) >= 2;
    }
    if (vo) {
        std::vector<uint8_t> sel(n > 0 ? n : 1);
        pr_vo_select(depth, n, th_depth, sel.data());
        float Ow[3];
        centre(Tl, Ow);
        const float invfx = 1.0f / C.fx, invfy = 1.0f / C.fy;
        for (int i = 0; i < n; ++i) {
            if (!sel[i] || (P[i].state & 7) >= 2) continue;
            const float z = depth[i];
            const float x3Dc[3] = {(kps[i].x - C.cx) * z * invfx, (kps[i].y - C.cy) * z * invfy, z};
            const float Rwc[9] = {Tl.R[0], Tl.R[3], Tl.R[6], Tl.R[1], Tl.R[4], Tl.R[7], Tl.R[2], Tl.R[5], Tl.R[8]};
            float X[3];
            affine(Rwc, x3Dc, Ow, X);
            P[i].x = X[0]; P[i].y = X[1]; P[i].z = X[2];
            P[i].state = (P[i].state & 8) | 1;
            D[i] = desc + (size_t)i * 32;
            blocks[i] = 0;
        }
    }
    float twc[3], tlc[3];
    centre(Tc, twc);
    affine(Tl.R, twc, Tl.t, tlc);
    const float mb = C.bf / C.fx;
    const bool bForward = tlc[2] > mb && !mono;
    const bool bBackward = -tlc[2] > mb && !mono;
    int nq = 0;
    for (int i = 0; i < n; ++i) {
        if ((P[i].state & 7) == 0 || (P[i].state & 8)) continue;
        const float x3Dw[3] = {P[i].x, P[i].y, P[i].z};
        float x3Dc[3];
        affine(Tc.R, x3Dw, Tc.t, x3Dc);
        if (!(x3Dc[2] > 0.f)) continue;
        const float invzc = 1.0 / (double)x3Dc[2];
        const float u = C.fx * x3Dc[0] * invzc + C.cx;
        const float v = C.fy * x3Dc[1] * invzc + C.cy;
        if (!(u >= bounds[0] && u <= bounds[2] && v >= bounds[1] && v <= bounds[3])) continue;
        const int o = kps[i].octave;
        PslProjQuery r;
        r.u = u;
        r.v = v;
        r.radius = th * scale[std::min(std::max(o, 0), nlevels - 1)];
        r.ur = u - C.bf * invzc;
        if (bForward) { r.min_level = o; r.max_level = -1; }
        else if (bBackward) { r.min_level = 0; r.max_level = o; }
        else { r.min_level = o - 1; r.max_level = o + 1; }
        r.angle = kps[i].angle;
        r.blocks = blocks[i];
        q[nq] = r;
        memcpy(qdesc + (size_t)nq * 32, D[i], 32);
        owner[nq] = i;
        ++nq;
    }
    return nq;
}

int pr_project_frustum(const PslPose* Tcw, const PslMapPointGeom* mp, const uint8_t* mpdesc, int nmp, const PslCamera* cam,
                       const float* scale, int nlevels, float log_scale_factor, float view_cos_limit, float th, const float* bounds,
                       PslProjQuery* q, uint8_t* qdesc, int32_t* owner, uint8_t* inview, int32_t* level, float* viewcos) {
    const PslCamera& C = *cam;
    float Ow[3];
    centre(*Tcw, Ow);
    int nq = 0;
    for (int j = 0; j < nmp; ++j) {
        const PslMapPointGeom& G = mp[j];
        inview[j] = 0; level[j] = -1; viewcos[j] = 0.f;
        const float P[3] = {G.x, G.y, G.z};
        float Pc[3];
        affine(Tcw->R, P, Tcw->t, Pc);
        if (!(Pc[2] > 0.f)) continue;
        const float invz = 1.0f / Pc[2];
        const float u = C.fx * Pc[0] * invz + C.cx;
        const float v = C.fy * Pc[1] * invz + C.cy;
        if (!(u >= bounds[0] && u <= bounds[2] && v >= bounds[1] && v <= bounds[3])) continue;
        const float maxDistance = 1.2f * G.max_dist, minDistance = 0.8f * G.min_dist;
        const float PO[3] = {P[0] - Ow[0], P[1] - Ow[1], P[2] - Ow[2]};
        const float dist = (float)sqrt((double)PO[0] * PO[0] + (double)PO[1] * PO[1] + (double)PO[2] * PO[2]);
        if (dist < minDistance || dist > maxDistance) continue;
        const double dot = (double)PO[0] * G.nx + (double)PO[1] * G.ny + (double)PO[2] * G.nz;
        const float viewCos = (float)(dot / (double)dist);
        if (viewCos < view_cos_limit) continue;
        const int lvl = predict_level(G.max_dist / dist, log_scale_factor, nlevels, 0);
        float r = viewCos > 0.998 ? 2.5f : 4.0f;
        if (th != 1.0f) r *= th;
        inview[j] = 1; level[j] = lvl; viewcos[j] = viewCos;
        PslProjQuery e;
        e.u = u;
        e.v = v;
        e.radius = r * scale[lvl];
        e.ur = u - C.bf * invz;
        e.min_level = lvl - 1;
        e.max_level = lvl;
        e.angle = 0.f;
        e.blocks = 1;
        q[nq] = e;
        memcpy(qdesc + (size_t)nq * 32, mpdesc + (size_t)j * 32, 32);
        owner[nq] = j;
        ++nq;
    }
    return nq;
}

}  // extern "C"
