// The host side of tools/bench_map_upkeep.py: MapPoint::UpdateNormalAndDepth and MapLine::UpdateAverageDir as plain C++ loops over the
// arrays the library takes, one row after the other on one core, with the arithmetic of include/pslfe.h (built with -ffp-contract=off).
// Written for that tool, as the baseline a caller's own host loop stands for; it is not product code and not the reference's code.
#include <math.h>
#include <stdint.h>

#include "../include/pslfe.h"

static float norm3(float a, float b, float c, double* as_double) {
    double s = (double)a * (double)a;
    s += (double)b * (double)b;
    s += (double)c * (double)c;
    const double n = sqrt(s);
    if (as_double) *as_double = n;
    return (float)n;
}

extern "C" void host_update_normal_and_depth(PslMapPointGeom* mp, int M, const int32_t* obs_off, const int32_t* obs_kf, const float* centres,
                                             const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* skip, const float* scale,
                                             int nlevels) {
    for (int i = 0; i < M; ++i) {
        const int b = obs_off[i], e = obs_off[i + 1];
        if (e <= b || (skip && skip[i])) continue;
        const float P[3] = {mp[i].x, mp[i].y, mp[i].z};
        float normal[3] = {0.f, 0.f, 0.f};
        for (int o = b; o < e; ++o) {
            const float* ow = centres + 3 * (size_t)obs_kf[o];
            const float n0 = P[0] - ow[0], n1 = P[1] - ow[1], n2 = P[2] - ow[2];
            double nrm;
            norm3(n0, n1, n2, &nrm);
            const float t = (float)(1.0 / nrm);
            normal[0] += n0 * t; normal[1] += n1 * t; normal[2] += n2 * t;
        }
        const float t = (float)(1.0 / (double)(e - b));
        const float* ow = centres + 3 * (size_t)ref_kf[i];
        const float dist = norm3(P[0] - ow[0], P[1] - ow[1], P[2] - ow[2], nullptr);
        mp[i].nx = normal[0] * t; mp[i].ny = normal[1] * t; mp[i].nz = normal[2] * t;
        mp[i].max_dist = dist * scale[ref_level[i]];
        mp[i].min_dist = mp[i].max_dist / scale[nlevels - 1];
    }
}

extern "C" void host_line_update_average_dir(PslMapLineGeom* ml, int M, const int32_t* obs_off, const int32_t* obs_kf, const float* centres,
                                             const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* skip, const float* scale,
                                             int nlevels) {
    for (int i = 0; i < M; ++i) {
        const int b = obs_off[i], e = obs_off[i + 1];
        if (e <= b || (skip && skip[i])) continue;
        double mid[3], normal[3] = {0.0, 0.0, 0.0};
        for (int c = 0; c < 3; ++c) mid[c] = 0.5 * (ml[i].sp[c] + ml[i].ep[c]);
        for (int o = b; o < e; ++o) {
            const float* ow = centres + 3 * (size_t)obs_kf[o];
            const double n0 = mid[0] - (double)ow[0], n1 = mid[1] - (double)ow[1], n2 = mid[2] - (double)ow[2];
            double s = n0 * n0;
            s += n1 * n1;
            s += n2 * n2;
            const double nrm = sqrt(s);
            normal[0] += n0 / nrm; normal[1] += n1 / nrm; normal[2] += n2 / nrm;
        }
        const float* ow = centres + 3 * (size_t)ref_kf[i];
        float cm[3];
        for (int c = 0; c < 3; ++c) cm[c] = (0.5f * (float)ml[i].sp[c] + 0.5f * (float)ml[i].ep[c]) - ow[c];
        const float dist = norm3(cm[0], cm[1], cm[2], nullptr);
        for (int c = 0; c < 3; ++c) ml[i].normal[c] = normal[c] / (double)(e - b);
        ml[i].max_dist = dist * scale[ref_level[i]];
        ml[i].min_dist = ml[i].max_dist / scale[nlevels - 1];
    }
}
