// The bodies of LocalMapping::CreateNewMapPoints (src/LocalMapping.cc:354-517) and CreateNewMapLines2 (:599-755) for one matched pair,
// as functions of one thread, and the plain one-core loops over neighbours built on them.  Product code.  Plain C++ text: the kernels
// (pslfe_kf.hip, pslfe_kf_line.hip) include it for the device and tools/dropin/newpoints_main.cpp for its host loop (define
// PSL_TRI_HOST_ONLY there to build with g++ alone, without the library), so both run the same single IEEE operations (build with
// -ffp-contract=off).  tests/new_points_cases.py is the same text in numpy.
//
// Conventions: those stated above PslPose in include/pslfe.h.
//   Rwc*xn, Rwc*x3Dc + Ow, -Rcw.t()*tcw   every row the double sum, in index order, of the exact products (+ the double of the addend),
//                                          rounded once to float
//   Mat::dot, cv::norm                     double sums in index order; norm takes the double sqrt
//   row.dot(x3Dt) + t assigned to a float  the double dot + the double of t, rounded once
//   ray1.dot(ray2)/(norm*norm)             a double product, a double division, rounded to float
//   x*row - row (A.row(i))                 float operations (as psl_init_rt_row of initializer_kernels.h)
//   cv::SVD::compute, CV_32F, FULL_UV      psl_init_jacobi of initializer_kernels.h on At = A^T; vt.row(3) needs no completion
//   x3D.rowRange(0,3)/x3D[3]               times 1.0 / x3D[3] in double, rounded to float
//   cos(2*atan2(mb/2, depth))              the float overloads: add_inc/LineExtractor.h:17 (through include/Frame.h:32) puts `using
//                                          namespace std` in front of src/LocalMapping.cc, so the calls resolve to std::atan2(float,
//                                          float) and std::cos(float): psl_atan2f, a float doubling, psl_sincosf
//   1.0/z                                  the double quotient rounded to float
//   5.991*sigma2, 7.8*sigma2               double products; the float error sum is widened for the comparison
//   every other step                       the reference's float operation, in its order, never contracted
// Kept as written: the right-image term of the SECOND keyframe uses mpCurrentKeyFrame->mbf (:474); bStereo2 of a line pair is read from
// the CURRENT keyframe's mvLineEq[idx2] (:607).  Where idx2 is not a line of the current keyframe the reference reads out of range; the
// library drops the pair with PSL_TRIL_IDX2_RANGE.  KeyFrame::UnprojectStereo returns an empty Mat for z <= 0, on which the reference
// would throw at x3D.t(): PSL_TRI_UNPROJECT_EMPTY.  An octave indexes the level tables modulo 16 (tables padded with zeros), as the
// search does.
#ifndef PSL_TRIANGULATE_KERNELS_H
#define PSL_TRIANGULATE_KERNELS_H

#include "../../include/pslfe.h"
#include "psl_device_math.h"
#include "initializer_kernels.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

#define PSL_TRI_HD __attribute__((always_inline)) PSL_PO_HD
#define PSL_TRI_LEVELS 16
#define PSL_TRI_WS_F 32   // floats of SVD workspace per row: At 16, Vt 16
#define PSL_TRI_WS_D 4    // doubles: W
#define PSL_TRI_AT(p, k) (p)[(size_t)(k) * ES]

// A keyframe as both bodies read it
struct PslTriCam {
    float Rcw[9], tcw[3], Ow[3];
    float fx, fy, cx, cy, invfx, invfy, mb;
};
PSL_TRI_HD float psl_tri_affine(float m0, float m1, float m2, float x0, float x1, float x2, float t) {
    double a = PSL_DMUL((double)m0, (double)x0);
    a = PSL_DADD(a, PSL_DMUL((double)m1, (double)x1));
    a = PSL_DADD(a, PSL_DMUL((double)m2, (double)x2));
    a = PSL_DADD(a, (double)t);
    return (float)a;
}
PSL_TRI_HD double psl_tri_dot(const float* a, const float* b) {
    double s = PSL_DMUL((double)a[0], (double)b[0]);
    s = PSL_DADD(s, PSL_DMUL((double)a[1], (double)b[1]));
    return PSL_DADD(s, PSL_DMUL((double)a[2], (double)b[2]));
}
PSL_TRI_HD double psl_tri_norm_d(const float* a) { return PSL_PO_SQRT(psl_tri_dot(a, a)); }
PSL_TRI_HD void psl_tri_cam_setup(const PslPose* T, float fx, float fy, float cx, float cy, float mb, PslTriCam* C) {
    for (int i = 0; i < 9; ++i) C->Rcw[i] = T->R[i];
    for (int i = 0; i < 3; ++i) C->tcw[i] = T->t[i];
    for (int r = 0; r < 3; ++r) C->Ow[r] = -psl_tri_affine(T->R[r], T->R[3 + r], T->R[6 + r], T->t[0], T->t[1], T->t[2], 0.f);
    C->fx = fx; C->fy = fy; C->cx = cx; C->cy = cy; C->mb = mb;
    C->invfx = PSL_FDIV(1.0f, fx); C->invfy = PSL_FDIV(1.0f, fy);
}
// Twc.rowRange(0,3).colRange(0,3)*xc + Twc.rowRange(0,3).col(3)
PSL_TRI_HD void psl_tri_to_world(const PslTriCam* C, float x, float y, float z, float* w) {
    for (int r = 0; r < 3; ++r) w[r] = psl_tri_affine(C->Rcw[r], C->Rcw[3 + r], C->Rcw[6 + r], x, y, z, C->Ow[r]);
}
// Rcw.row(r).dot(x3Dt) + tcw(r), assigned to a float
PSL_TRI_HD float psl_tri_cam_row(const PslTriCam* C, int r, const float* p) {
    return (float)PSL_DADD(psl_tri_dot(C->Rcw + 3 * r, p), (double)C->tcw[r]);
}
// cv::norm(p - Ow) assigned to a float
PSL_TRI_HD float psl_tri_dist(const PslTriCam* C, const float* p) {
    const float n[3] = {PSL_FSUB(p[0], C->Ow[0]), PSL_FSUB(p[1], C->Ow[1]), PSL_FSUB(p[2], C->Ow[2])};
    return (float)psl_tri_norm_d(n);
}
// the monocular gate of one end point or keypoint: 1 = rejected
PSL_TRI_HD int psl_tri_reproj_mono(const PslTriCam* C, const float* p, float z, float u0, float v0, float sigma2) {
    const float x = psl_tri_cam_row(C, 0, p), y = psl_tri_cam_row(C, 1, p);
    const float invz = (float)PSL_PO_DIV(1.0, (double)z);
    const float u = PSL_FADD(PSL_FMUL(PSL_FMUL(C->fx, x), invz), C->cx), v = PSL_FADD(PSL_FMUL(PSL_FMUL(C->fy, y), invz), C->cy);
    const float ex = PSL_FSUB(u, u0), ey = PSL_FSUB(v, v0);
    return (double)PSL_FADD(PSL_FMUL(ex, ex), PSL_FMUL(ey, ey)) > PSL_DMUL(5.991, (double)sigma2);
}
PSL_TRI_HD int psl_tri_reproj_stereo(const PslTriCam* C, float mbf, const float* p, float z, float u0, float v0, float ur0, float sigma2) {
    const float x = psl_tri_cam_row(C, 0, p), y = psl_tri_cam_row(C, 1, p);
    const float invz = (float)PSL_PO_DIV(1.0, (double)z);
    const float u = PSL_FADD(PSL_FMUL(PSL_FMUL(C->fx, x), invz), C->cx);
    const float ur = PSL_FSUB(u, PSL_FMUL(mbf, invz));
    const float v = PSL_FADD(PSL_FMUL(PSL_FMUL(C->fy, y), invz), C->cy);
    const float ex = PSL_FSUB(u, u0), ey = PSL_FSUB(v, v0), er = PSL_FSUB(ur, ur0);
    return (double)PSL_FADD(PSL_FADD(PSL_FMUL(ex, ex), PSL_FMUL(ey, ey)), PSL_FMUL(er, er)) > PSL_DMUL(7.8, (double)sigma2);
}
// :498 / :733
PSL_TRI_HD int psl_tri_ratio_out(float ratioDist, float ratioFactor, float ratioOctave) {
    return PSL_FMUL(ratioDist, ratioFactor) < ratioOctave || ratioDist > PSL_FMUL(ratioOctave, ratioFactor);
}

// One keypoint of a matched pair: mvKeysUn[idx].pt / .octave, mvKeys[idx].pt (the raw keypoint of UnprojectStereo), mvuRight, mvDepth
struct PslTriObs {
    float ux, uy, rx, ry, uright, depth;
    int octave;
};

// ---- CreateNewMapPoints :354-499 for one pair: PSL_TRI_* status, x3d written for every status that has one (zeros otherwise) -------
// C1: mpCurrentKeyFrame, C2: pKF2; mbf1 = mpCurrentKeyFrame->mbf; sf / sig2: PSL_TRI_LEVELS entries; a: PSL_TRI_WS_F floats, w:
// PSL_TRI_WS_D doubles of workspace, element k at [k * ES].
template <int ES>
PSL_TRI_HD int psl_tri_point_row(const PslTriCam* C1, const PslTriCam* C2, float mbf1, const PslTriObs* o1, const PslTriObs* o2, const float* sf,
                                 const float* sig2, float ratioFactor, float* a, double* w, float* x3d) {
    x3d[0] = x3d[1] = x3d[2] = 0.f;
    const bool bStereo1 = o1->uright >= 0, bStereo2 = o2->uright >= 0;
    const float xn1[3] = {PSL_FMUL(PSL_FSUB(o1->ux, C1->cx), C1->invfx), PSL_FMUL(PSL_FSUB(o1->uy, C1->cy), C1->invfy), 1.0f};
    const float xn2[3] = {PSL_FMUL(PSL_FSUB(o2->ux, C2->cx), C2->invfx), PSL_FMUL(PSL_FSUB(o2->uy, C2->cy), C2->invfy), 1.0f};
    float ray1[3], ray2[3];
    for (int r = 0; r < 3; ++r) {   // Rwc = Rcw.t()
        ray1[r] = psl_tri_affine(C1->Rcw[r], C1->Rcw[3 + r], C1->Rcw[6 + r], xn1[0], xn1[1], xn1[2], 0.f);
        ray2[r] = psl_tri_affine(C2->Rcw[r], C2->Rcw[3 + r], C2->Rcw[6 + r], xn2[0], xn2[1], xn2[2], 0.f);
    }
    const float cosParallaxRays = (float)PSL_PO_DIV(psl_tri_dot(ray1, ray2), PSL_DMUL(psl_tri_norm_d(ray1), psl_tri_norm_d(ray2)));
    const float cosParallaxStereo0 = PSL_FADD(cosParallaxRays, 1.0f);
    float cosParallaxStereo1 = cosParallaxStereo0, cosParallaxStereo2 = cosParallaxStereo0;
    if (bStereo1 || bStereo2) {
        const float ang = PSL_FMUL(2.0f, bStereo1 ? psl_atan2f(PSL_FDIV(C1->mb, 2.0f), o1->depth) : psl_atan2f(PSL_FDIV(C2->mb, 2.0f), o2->depth));
        float sn, cs;
        psl_sincosf(ang, &sn, &cs);
        if (bStereo1) cosParallaxStereo1 = cs; else cosParallaxStereo2 = cs;
    }
    const float cosParallaxStereo = cosParallaxStereo2 < cosParallaxStereo1 ? cosParallaxStereo2 : cosParallaxStereo1;   // std::min
    float p[3];
    if (cosParallaxRays < cosParallaxStereo && cosParallaxRays > 0 && (bStereo1 || bStereo2 || (double)cosParallaxRays < 0.9998)) {
        float* v = a + (size_t)16 * ES;
        const float* T1 = C1->Rcw; const float* T2 = C2->Rcw;
        for (int j = 0; j < 4; ++j) {   // At = A^T; column j of Tcw: R[.][j], j == 3: tcw
            const float r10 = j < 3 ? T1[j] : C1->tcw[0], r11 = j < 3 ? T1[3 + j] : C1->tcw[1], r12 = j < 3 ? T1[6 + j] : C1->tcw[2];
            const float r20 = j < 3 ? T2[j] : C2->tcw[0], r21 = j < 3 ? T2[3 + j] : C2->tcw[1], r22 = j < 3 ? T2[6 + j] : C2->tcw[2];
            PSL_TRI_AT(a, 4 * j + 0) = PSL_FSUB(PSL_FMUL(xn1[0], r12), r10);
            PSL_TRI_AT(a, 4 * j + 1) = PSL_FSUB(PSL_FMUL(xn1[1], r12), r11);
            PSL_TRI_AT(a, 4 * j + 2) = PSL_FSUB(PSL_FMUL(xn2[0], r22), r20);
            PSL_TRI_AT(a, 4 * j + 3) = PSL_FSUB(PSL_FMUL(xn2[1], r22), r21);
        }
        psl_init_jacobi<ES>(a, 4, 4, w, v);
        const float w3 = PSL_TRI_AT(v, 15);
        if (w3 == 0) return PSL_TRI_W_ZERO;
        const double inv = PSL_PO_DIV(1.0, (double)w3);
        for (int k = 0; k < 3; ++k) p[k] = (float)PSL_DMUL((double)PSL_TRI_AT(v, 12 + k), inv);
    } else if (bStereo1 && cosParallaxStereo1 < cosParallaxStereo2) {
        const float z = o1->depth;
        if (!(z > 0)) return PSL_TRI_UNPROJECT_EMPTY;
        psl_tri_to_world(C1, PSL_FMUL(PSL_FMUL(PSL_FSUB(o1->rx, C1->cx), z), C1->invfx), PSL_FMUL(PSL_FMUL(PSL_FSUB(o1->ry, C1->cy), z), C1->invfy), z, p);
    } else if (bStereo2 && cosParallaxStereo2 < cosParallaxStereo1) {
        const float z = o2->depth;
        if (!(z > 0)) return PSL_TRI_UNPROJECT_EMPTY;
        psl_tri_to_world(C2, PSL_FMUL(PSL_FMUL(PSL_FSUB(o2->rx, C2->cx), z), C2->invfx), PSL_FMUL(PSL_FMUL(PSL_FSUB(o2->ry, C2->cy), z), C2->invfy), z, p);
    } else {
        return PSL_TRI_LOW_PARALLAX;
    }
    x3d[0] = p[0]; x3d[1] = p[1]; x3d[2] = p[2];
    const float z1 = psl_tri_cam_row(C1, 2, p);
    if (z1 <= 0) return PSL_TRI_DEPTH1;
    const float z2 = psl_tri_cam_row(C2, 2, p);
    if (z2 <= 0) return PSL_TRI_DEPTH2;
    const float sigmaSquare1 = sig2[o1->octave & (PSL_TRI_LEVELS - 1)];
    if (!bStereo1) {
        if (psl_tri_reproj_mono(C1, p, z1, o1->ux, o1->uy, sigmaSquare1)) return PSL_TRI_REPROJ1_MONO;
    } else {
        if (psl_tri_reproj_stereo(C1, mbf1, p, z1, o1->ux, o1->uy, o1->uright, sigmaSquare1)) return PSL_TRI_REPROJ1_STEREO;
    }
    const float sigmaSquare2 = sig2[o2->octave & (PSL_TRI_LEVELS - 1)];
    if (!bStereo2) {
        if (psl_tri_reproj_mono(C2, p, z2, o2->ux, o2->uy, sigmaSquare2)) return PSL_TRI_REPROJ2_MONO;
    } else {   // mpCurrentKeyFrame->mbf, :474
        if (psl_tri_reproj_stereo(C2, mbf1, p, z2, o2->ux, o2->uy, o2->uright, sigmaSquare2)) return PSL_TRI_REPROJ2_STEREO;
    }
    const float dist1 = psl_tri_dist(C1, p), dist2 = psl_tri_dist(C2, p);
    if (dist1 == 0 || dist2 == 0) return PSL_TRI_DIST_ZERO;
    const float ratioDist = PSL_FDIV(dist2, dist1);
    const float ratioOctave = PSL_FDIV(sf[o1->octave & (PSL_TRI_LEVELS - 1)], sf[o2->octave & (PSL_TRI_LEVELS - 1)]);
    if (psl_tri_ratio_out(ratioDist, ratioFactor, ratioOctave)) return PSL_TRI_RATIO;
    return PSL_TRI_CREATED;
}

// ---- CreateNewMapLines2 :599-735 for one pair ---------------------------------------------------------------------------------------
// kl1 / kl2: the keylines; l3d1 / l3d2: mvLines3D[idx1] of the current keyframe / mvLines3D[idx2] of pKF2 (6 doubles, camera frame);
// stereo1 = mvLineEq[idx1][2] > 0 and stereo2 = mvLineEq[idx2][2] > 0, BOTH of the current keyframe (the caller has checked idx2's range).
PSL_TRI_HD void psl_tri_obtain_line(const PslTriCam* C, const double* l3d, float* sp, float* ep) {
    psl_tri_to_world(C, (float)l3d[0], (float)l3d[1], (float)l3d[2], sp);
    psl_tri_to_world(C, (float)l3d[3], (float)l3d[4], (float)l3d[5], ep);
}
PSL_TRI_HD int psl_tri_line_row(const PslTriCam* C1, const PslTriCam* C2, const PslKeyLine* kl1, const PslKeyLine* kl2, const double* l3d1,
                                const double* l3d2, int stereo1, int stereo2, const float* sf, const float* sig2, float ratioFactor, float* sp,
                                float* ep) {
    sp[0] = sp[1] = sp[2] = ep[0] = ep[1] = ep[2] = 0.f;
    if (stereo1) psl_tri_obtain_line(C1, l3d1, sp, ep);
    else if (stereo2) psl_tri_obtain_line(C2, l3d2, sp, ep);
    else return PSL_TRIL_NO_STEREO;
    const float zsp1 = psl_tri_cam_row(C1, 2, sp);
    if (zsp1 <= 0) return PSL_TRIL_DEPTH_SP1;
    const float zep1 = psl_tri_cam_row(C1, 2, ep);
    if (zep1 <= 0) return PSL_TRIL_DEPTH_EP1;
    const float zsp2 = psl_tri_cam_row(C2, 2, sp);
    if (zsp2 <= 0) return PSL_TRIL_DEPTH_SP2;
    const float zep2 = psl_tri_cam_row(C2, 2, ep);
    if (zep2 <= 0) return PSL_TRIL_DEPTH_EP2;
    const float sigmaSquare1 = sig2[kl1->octave & (PSL_TRI_LEVELS - 1)];
    if (psl_tri_reproj_mono(C1, sp, zsp1, kl1->startPointX, kl1->startPointY, sigmaSquare1)) return PSL_TRIL_REPROJ_SP1;
    if (psl_tri_reproj_mono(C1, ep, zep1, kl1->endPointX, kl1->endPointY, sigmaSquare1)) return PSL_TRIL_REPROJ_EP1;
    const float sigmaSquare2 = sig2[kl2->octave & (PSL_TRI_LEVELS - 1)];
    if (psl_tri_reproj_mono(C2, sp, zsp2, kl2->startPointX, kl2->startPointY, sigmaSquare2)) return PSL_TRIL_REPROJ_SP2;
    if (psl_tri_reproj_mono(C2, ep, zep2, kl2->endPointX, kl2->endPointY, sigmaSquare2)) return PSL_TRIL_REPROJ_EP2;
    const float distsp1 = psl_tri_dist(C1, sp), distep1 = psl_tri_dist(C1, ep), distsp2 = psl_tri_dist(C2, sp), distep2 = psl_tri_dist(C2, ep);
    if (distsp1 == 0 || distep1 == 0 || distsp2 == 0 || distep2 == 0) return PSL_TRIL_DIST_ZERO;
    const float ratioDistsp = PSL_FDIV(distsp2, distsp1), ratioDistep = PSL_FDIV(distep2, distep1);
    const float ratioOctave = PSL_FDIV(sf[kl1->octave & (PSL_TRI_LEVELS - 1)], sf[kl2->octave & (PSL_TRI_LEVELS - 1)]);
    if (psl_tri_ratio_out(ratioDistsp, ratioFactor, ratioOctave) || psl_tri_ratio_out(ratioDistep, ratioFactor, ratioOctave)) return PSL_TRIL_RATIO;
    return PSL_TRIL_CREATED;
}
// the walk of one line of the current keyframe over the neighbours in order: match0 = the search's rows at the call (stride n1), the
// filter GetMapLine(i) of LSDmatcher::SearchForTriangulation as neighbour k sees it.  cams: K set-up neighbours.  Outputs at k*n1 + i.
struct PslTriLineSet {
    const PslTriCam* C1;
    const PslTriCam* cams;            // [K]
    const PslTriNeighbour* nb;        // [K]
    int K, n1;
    const PslKeyLine* kls1;
    const double* l3d1;               // [n1][6]
    const float* lineeq1;             // [n1]
    const PslKeyLine* kls2;
    const double* l3d2;
    const int32_t* off2;              // [K+1]
    const int32_t* match0;
    float sf[PSL_TRI_LEVELS], sig2[PSL_TRI_LEVELS];
    float ratioFactor;
    int32_t* match;
    int32_t* status;
    float* sp;
    float* ep;
    int32_t* created_by;
};
PSL_TRI_HD void psl_tri_line_walk(const PslTriLineSet* S, int i) {
    int by = -1;
    for (int k = 0; k < S->K; ++k) {
        const size_t row = (size_t)k * S->n1 + i;
        float sp[3] = {0.f, 0.f, 0.f}, ep[3] = {0.f, 0.f, 0.f};
        int st, m = -1;
        const int n2 = S->off2[k + 1] - S->off2[k];
        const int j = S->match0[row];
        if (!S->nb[k].active) st = PSL_TRIL_INACTIVE;
        else if (j < 0 || j >= n2) st = PSL_TRIL_NO_MATCH;
        else if (by >= 0) st = PSL_TRIL_TAKEN;
        else {
            m = j;
            if (j >= S->n1) st = PSL_TRIL_IDX2_RANGE;
            else
                st = psl_tri_line_row(S->C1, S->cams + k, S->kls1 + i, S->kls2 + S->off2[k] + j, S->l3d1 + (size_t)6 * i,
                                      S->l3d2 + (size_t)6 * (S->off2[k] + j), S->lineeq1[i] > 0, S->lineeq1[j] > 0, S->sf, S->sig2, S->ratioFactor, sp, ep);
            if (st == PSL_TRIL_CREATED) by = k;
        }
        S->match[row] = m; S->status[row] = st;
        for (int c = 0; c < 3; ++c) { S->sp[3 * row + c] = sp[c]; S->ep[3 * row + c] = ep[c]; }
    }
    S->created_by[i] = by;
}

#ifndef __HIP_DEVICE_COMPILE__
// ---- the loops of one core ------------------------------------------------------------------------------------------------------------
// NOTE: the search exists twice.  The "one text" of this header is the pair arithmetic above; the candidate loop, the rotation bin and
// ComputeThreeMaxima below are a second, sequential writing of psl_tri_choice_row (pslfe_kf.hip), psl_rot_bin and psl_three_maxima
// (match_kernels.h), which are wave-parallel device code.  Nothing but the tests keeps the two equal: tests/test_new_points_gpu.py
// compares the compiled consumer's loop with the kernels, tests/test_new_points_cpu.py this loop with oracle/kf_oracle.cpp's.
// ORBmatcher::SearchForTriangulation (src/ORBmatcher.cc:657-823) of one neighbour as pslfe_kf_search_for_triangulation states it, with
// skip[q] != 0 <=> the feature of query q has a map point by now (:699-703): match[q] = idx2 or -1; returns nmatches.
static inline int psl_tri_hamming(const uint8_t* a, const uint8_t* b) {
    int d = 0;
    for (int k = 0; k < 32; ++k) d += __builtin_popcount((unsigned)(a[k] ^ b[k]));
    return d;
}
static inline int psl_tri_rot_bin(float a1, float a2) {
    float rot = a1 - a2;
    if (rot < 0.0f) rot = rot + 360.0f;
    int bin = (int)__builtin_roundf(rot * (1.0f / 30));
    if (bin == 30) bin = 0;
    return bin < 0 ? 0 : (bin >= 30 ? 29 : bin);
}
static inline int psl_tri_search_host(const PslKeyPoint* kps2, const uint8_t* desc2, const float* uright2, int n2, const int32_t* fidx2, int nfidx2,
                                      const uint8_t* taken2, const PslTriQuery* q, const uint8_t* qdesc, const uint8_t* skip, int nq, const float* F,
                                      float ex, float ey, int only_stereo, int check_ori, const float* sf, const float* sig2, int32_t* match) {
    int hist[30];
    for (int b = 0; b < 30; ++b) hist[b] = 0;
    for (int qi = 0; qi < nq; ++qi) {
        match[qi] = -1;
        if (skip[qi]) continue;
        const float a = (q[qi].x * F[0] + q[qi].y * F[3]) + F[6], b = (q[qi].x * F[1] + q[qi].y * F[4]) + F[7], c = (q[qi].x * F[2] + q[qi].y * F[5]) + F[8];
        const float den = a * a + b * b;
        const int start = q[qi].start > 0 ? q[qi].start : 0, len = q[qi].len < nfidx2 - start ? q[qi].len : nfidx2 - start;
        int bestDist = 50, bestIdx2 = -1;
        for (int j = 0; j < len; ++j) {
            const int idx2 = fidx2[start + j];
            if (idx2 < 0 || idx2 >= n2 || taken2[idx2]) continue;
            const bool stereo2 = uright2[idx2] >= 0;
            if (only_stereo && !stereo2) continue;
            const int dist = psl_tri_hamming(qdesc + (size_t)qi * 32, desc2 + (size_t)idx2 * 32);
            if (dist > 50 || dist > bestDist) continue;
            const int octave = kps2[idx2].octave & (PSL_TRI_LEVELS - 1);
            if (!q[qi].stereo && !stereo2) {
                const float dx = ex - kps2[idx2].x, dy = ey - kps2[idx2].y;
                if (dx * dx + dy * dy < 100.0f * sf[octave]) continue;
            }
            const float num = (a * kps2[idx2].x + b * kps2[idx2].y) + c;
            if (den == 0) continue;
            const float dsqr = (num * num) / den;
            if (!((double)dsqr < 3.84 * (double)sig2[octave])) continue;
            bestIdx2 = idx2; bestDist = dist;
        }
        match[qi] = bestIdx2;
        if (bestIdx2 >= 0 && check_ori) ++hist[psl_tri_rot_bin(q[qi].angle, kps2[bestIdx2].angle)];
    }
    int nm = 0;
    if (check_ori) {
        int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
        for (int i = 0; i < 30; ++i) {
            const int sz = hist[i];
            if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
            else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
            else if (sz > max3) { max3 = sz; ind3 = i; }
        }
        if ((float)max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
        else if ((float)max3 < 0.1f * (float)max1) ind3 = -1;
        for (int qi = 0; qi < nq; ++qi) {
            if (match[qi] < 0) continue;
            const int bin = psl_tri_rot_bin(q[qi].angle, kps2[match[qi]].angle);
            if (bin != ind1 && bin != ind2 && bin != ind3) match[qi] = -1;
        }
    }
    for (int qi = 0; qi < nq; ++qi) nm += match[qi] >= 0;
    return nm;
}

// One keyframe of the frame store as the host loop reads it
struct PslTriHostKf {
    const PslKeyPoint* kps;   // mvKeysUn
    const uint8_t* desc;
    const float* uright;
    int n;
};
// The arrays of pslfe_kf_create_new_map_points on the host; kf2[k] = the slot of neighbour k
struct PslTriPointSet {
    const PslTriKeyFrame* kf1;
    int N1;
    const PslKeyPoint* keysun1;
    const float* keys1;
    const float* uright1;
    const float* depth1;
    const uint8_t* taken1;
    const PslTriNeighbour* nb;
    int K;
    const PslTriHostKf* kf2;
    const int32_t* fidx2;
    const int32_t* fidx_off;
    const uint8_t* taken2;
    const float* keys2;
    const float* depth2;
    const int32_t* kp_off;
    const PslTriQuery* queries;
    const int32_t* idx1;
    const uint8_t* qdesc;
    const int32_t* nq;
    int nqmax, only_stereo, check_ori;
    const float* scale_factors;
    const float* level_sigma2;
    int nlevels;
};
// CreateNewMapPoints :305-519 as the reference writes it: neighbour after neighbour, the search with the map-point state of the moment,
// then the matched pairs in the order of vMatchedPairs (idx1 ascending).  Outputs as pslfe_kf_create_new_map_points; taken / skip / q_of:
// N1 + nqmax bytes and N1 ints of workspace.  Returns *nnew.
static inline int psl_tri_create_points_host(const PslTriPointSet* S, int32_t* match, int32_t* status, float* x3d, int32_t* nmatches,
                                             int32_t* created_by, PslNewMapPoint* newp, PslMapPointGeom* geom, uint8_t* taken, uint8_t* skip,
                                             int32_t* q_of) {
    float sf[PSL_TRI_LEVELS], sig2[PSL_TRI_LEVELS], ws[PSL_TRI_WS_F];
    double wd[PSL_TRI_WS_D];
    for (int i = 0; i < PSL_TRI_LEVELS; ++i) { sf[i] = i < S->nlevels ? S->scale_factors[i] : 0.f; sig2[i] = i < S->nlevels ? S->level_sigma2[i] : 0.f; }
    PslTriCam C1, C2;
    psl_tri_cam_setup(&S->kf1->Tcw, S->kf1->fx, S->kf1->fy, S->kf1->cx, S->kf1->cy, S->kf1->mb, &C1);
    for (int i = 0; i < S->N1; ++i) { taken[i] = S->taken1[i] != 0; created_by[i] = -1; }
    int nnew = 0;
    for (int k = 0; k < S->K; ++k) {
        const PslTriNeighbour* nb = S->nb + k;
        const size_t base = (size_t)k * S->nqmax;
        const int nq = S->nq[k] < 0 ? 0 : (S->nq[k] < S->nqmax ? S->nq[k] : S->nqmax);
        for (int q = 0; q < S->nqmax; ++q) {
            match[base + q] = -1;
            status[base + q] = nb->active && q < nq && taken[S->idx1[base + q]] ? PSL_TRI_TAKEN : (nb->active || q >= nq ? PSL_TRI_NO_MATCH : PSL_TRI_INACTIVE);
            x3d[3 * (base + q)] = x3d[3 * (base + q) + 1] = x3d[3 * (base + q) + 2] = 0.f;
        }
        nmatches[k] = 0;
        if (!nb->active) continue;
        for (int q = 0; q < nq; ++q) skip[q] = taken[S->idx1[base + q]];
        const PslTriHostKf* kf2 = S->kf2 + k;
        const int range2 = S->kp_off[k + 1] - S->kp_off[k];   // a keypoint without a row in taken2 / keys2 / depth2 is no candidate
        nmatches[k] = psl_tri_search_host(kf2->kps, kf2->desc, kf2->uright, kf2->n < range2 ? kf2->n : range2, S->fidx2 + S->fidx_off[k], S->fidx_off[k + 1] - S->fidx_off[k],
                                          S->taken2 + S->kp_off[k], S->queries + base, S->qdesc + base * 32, skip, nq, nb->F12, nb->ex, nb->ey,
                                          S->only_stereo, S->check_ori, sf, sig2, match + base);
        psl_tri_cam_setup(&nb->Tcw, nb->fx, nb->fy, nb->cx, nb->cy, nb->mb, &C2);
        for (int i = 0; i < S->N1; ++i) q_of[i] = -1;
        for (int q = 0; q < nq; ++q)
            if (match[base + q] >= 0) q_of[S->idx1[base + q]] = q;
        for (int i1 = 0; i1 < S->N1; ++i1) {
            const int q = q_of[i1];
            if (q < 0) continue;
            const int i2 = match[base + q];
            const PslTriObs o1 = {S->keysun1[i1].x, S->keysun1[i1].y, S->keys1[2 * i1], S->keys1[2 * i1 + 1], S->uright1[i1], S->depth1[i1], S->keysun1[i1].octave};
            const size_t g2 = (size_t)S->kp_off[k] + i2;
            const PslTriObs o2 = {kf2->kps[i2].x, kf2->kps[i2].y, S->keys2[2 * g2], S->keys2[2 * g2 + 1], kf2->uright[i2], S->depth2[g2], kf2->kps[i2].octave};
            const int st = psl_tri_point_row<1>(&C1, &C2, S->kf1->mbf, &o1, &o2, sf, sig2, S->kf1->ratio_factor, ws, wd, x3d + 3 * (base + q));
            status[base + q] = st;
            if (st != PSL_TRI_CREATED) continue;
            taken[i1] = 1; created_by[i1] = k;
            const float* p = x3d + 3 * (base + q);
            const PslNewMapPoint np = {p[0], p[1], p[2], k, i1, i2};
            newp[nnew] = np;
            if (geom) { const PslMapPointGeom g = {p[0], p[1], p[2], 0.f, 0.f, 0.f, 0.f, 0.f}; geom[nnew] = g; }
            ++nnew;
        }
    }
    return nnew;
}

// CreateNewMapLines2 :554-757 behind the search: psl_tri_line_walk for every line, then the list in creation order (k ascending, idx1
// ascending).  cams: K PslTriCam of workspace.  Returns *nnew; nmatches[k] = the pairs neighbour k's search returns.
static inline int psl_tri_create_lines_host(PslTriLineSet* S, const PslTriKeyFrame* kf1, const float* scale_factors, const float* level_sigma2,
                                            int nlevels, PslTriCam* cams, int32_t* nmatches, PslNewMapLine* newl, PslMapLineGeom* geom) {
    PslTriCam C1;
    psl_tri_cam_setup(&kf1->Tcw, kf1->fx, kf1->fy, kf1->cx, kf1->cy, kf1->mb, &C1);
    for (int k = 0; k < S->K; ++k) psl_tri_cam_setup(&S->nb[k].Tcw, S->nb[k].fx, S->nb[k].fy, S->nb[k].cx, S->nb[k].cy, S->nb[k].mb, cams + k);
    for (int i = 0; i < PSL_TRI_LEVELS; ++i) { S->sf[i] = i < nlevels ? scale_factors[i] : 0.f; S->sig2[i] = i < nlevels ? level_sigma2[i] : 0.f; }
    S->C1 = &C1; S->cams = cams; S->ratioFactor = kf1->ratio_factor;
    for (int i = 0; i < S->n1; ++i) psl_tri_line_walk(S, i);
    int nnew = 0;
    for (int k = 0; k < S->K; ++k) {
        nmatches[k] = 0;
        for (int i = 0; i < S->n1; ++i) {
            const size_t row = (size_t)k * S->n1 + i;
            nmatches[k] += S->match[row] >= 0;
            if (S->created_by[i] != k) continue;
            PslNewMapLine nl;
            PslMapLineGeom g;
            memset(&g, 0, sizeof(g));
            for (int c = 0; c < 3; ++c) { nl.sp[c] = S->sp[3 * row + c]; nl.ep[c] = S->ep[3 * row + c]; g.sp[c] = (double)nl.sp[c]; g.ep[c] = (double)nl.ep[c]; }
            nl.k = k; nl.idx1 = i; nl.idx2 = S->match[row];
            newl[nnew] = nl;
            if (geom) geom[nnew] = g;
            ++nnew;
        }
    }
    return nnew;
}
#endif   // !__HIP_DEVICE_COMPILE__

#endif
