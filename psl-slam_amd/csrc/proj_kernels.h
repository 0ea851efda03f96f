// Shared by pslfe_project.hip, pslfe_project_line.hip, pslfe_kf_project.hip and pslfe_kf_line.hip: the cv::Mat pose algebra of the
// projection conventions (include/pslfe.h) - the pose products, the camera centre, cv::norm, Mat::dot - both
// PredictScale variants, the descriptor copy and the workgroup compaction that keeps emitted rows in input order.  Which form of the
// reference uses which arithmetic on top of these is the table of DESIGN.md §5.0h.  Product code.
#ifndef PSL_PROJ_KERNELS_H
#define PSL_PROJ_KERNELS_H

#include <limits.h>

#include "pslfe_internal.h"
#include "psl_device_math.h"
#ifndef PSL_F64_QUAL
#define PSL_F64_QUAL __host__ __device__ static inline
#endif
#include "psl_f64math.h"

#if defined(__HIP_DEVICE_COMPILE__)
#define PSL_DDIV(a, b) __ddiv_rn((a), (b))
#define PSL_DSQRT(a) __dsqrt_rn(a)
#else
#define PSL_DDIV(a, b) ((a) / (b))
#define PSL_DSQRT(a) __builtin_sqrt(a)
#endif

// row r of M * x + t: double products (exact for float operands), summed in index order, one rounding
__device__ __forceinline__ float psl_affine_row(float m0, float m1, float m2, float x0, float x1, float x2, float t) {
    double a = PSL_DMUL((double)m0, (double)x0);
    a = PSL_DADD(a, PSL_DMUL((double)m1, (double)x1));
    a = PSL_DADD(a, PSL_DMUL((double)m2, (double)x2));
    a = PSL_DADD(a, (double)t);
    return (float)a;
}

// The pose products.  y = M*x + t, M row-major: world to camera with a PslPose's (R, t), camera 1 to camera 2 with Sim3's (sR21, t21).
__device__ __forceinline__ void psl_pose_mul(const float* M, const float* t, float x0, float x1, float x2, float* y) {
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = psl_affine_row(M[3 * r], M[3 * r + 1], M[3 * r + 2], x0, x1, x2, t[r]);
}
// y = M^T*x + t: camera to world with (Rcw, Ow) (Frame::UnprojectStereo)
__device__ __forceinline__ void psl_pose_mul_t(const float* M, const float* t, float x0, float x1, float x2, float* y) {
#pragma unroll
    for (int r = 0; r < 3; ++r) y[r] = psl_affine_row(M[r], M[3 + r], M[6 + r], x0, x1, x2, t[r]);
}

// -R^T * t (camera centre twc / mOw of Frame::UpdatePoseMatrices)
__device__ __forceinline__ void psl_centre(const PslPose& T, float* c) {
    const float zero[3] = {0.f, 0.f, 0.f};
    psl_pose_mul_t(T.R, zero, T.t[0], T.t[1], T.t[2], c);
#pragma unroll
    for (int r = 0; r < 3; ++r) c[r] = -c[r];
}

// cv::norm of a float 3-vector as the double it returns: the double sum of the exact squares in index order, sqrt in double
__device__ __forceinline__ double psl_norm3_d(float p0, float p1, float p2) {
    double s = PSL_DMUL((double)p0, (double)p0);
    s = PSL_DADD(s, PSL_DMUL((double)p1, (double)p1));
    s = PSL_DADD(s, PSL_DMUL((double)p2, (double)p2));
    return PSL_DSQRT(s);
}
// ... assigned to a float (`const float dist = cv::norm(PO)`)
__device__ __forceinline__ float psl_norm3(float p0, float p1, float p2) { return (float)psl_norm3_d(p0, p1, p2); }

// one component of 0.5*(SP+EP) on float Mats: the float sum of the exact halves, one rounding (include/pslfe.h above PslMapLineGeom)
__device__ __forceinline__ float psl_half_sum(float a, float b) { return PSL_FADD(PSL_FMUL(0.5f, a), PSL_FMUL(0.5f, b)); }

// Mat::dot of two float 3-vectors: the double sum in index order
__device__ __forceinline__ double psl_dot3(float p0, float p1, float p2, float n0, float n1, float n2) {
    double dot = PSL_DMUL((double)p0, (double)n0);
    dot = PSL_DADD(dot, PSL_DMUL((double)p1, (double)n1));
    dot = PSL_DADD(dot, PSL_DMUL((double)p2, (double)n2));
    return dot;
}

// MapPoint::PredictScale (src/MapPoint.cc:385-416, both overloads): ceil(log(mfMaxDistance / dist) / mfLogScaleFactor), clamped
__device__ __forceinline__ int psl_predict_level(float max_dist, float dist, float log_scale_factor, int nlevels) {
    const float ratio = PSL_FDIV(max_dist, dist);
    // psl_log needs a positive finite argument: log(0) = -inf -> level 0, log(inf) = inf -> the last level
    double ls = ratio > 0.f ? 1e300 : -1.0;
    if (ratio > 0.f && ratio < __builtin_huge_valf()) ls = __builtin_ceil(PSL_DDIV(psl_log((double)ratio), (double)log_scale_factor));
    return ls > 0.0 ? (ls < (double)nlevels ? (int)ls : nlevels - 1) : 0;
}

// ceil(logf(ratio) / lsf) of MapLine::PredictScale (add_src/MapLine.cpp:381-390), unclamped; logf = the correctly rounded float log;
// +inf -> INT_MAX, 0 -> INT_MIN, NaN -> 0
__device__ __forceinline__ int psl_line_level(float ratio, float lsf) {
    float lf;
    if (ratio != ratio) return 0;
    if (ratio > 0.f && ratio < __builtin_huge_valf()) lf = (float)psl_log((double)ratio);
    else lf = ratio > 0.f ? __builtin_huge_valf() : -__builtin_huge_valf();
    const float c = __builtin_ceilf(PSL_FDIV(lf, lsf));
    if (c != c) return 0;
    if (c >= 2147483648.f) return INT_MAX;
    if (c < -2147483648.f) return INT_MIN;
    return (int)c;
}

// one 32-byte descriptor row
__device__ __forceinline__ void psl_copy_desc(uint8_t* dst, const uint8_t* src) {
    const uint4* s = reinterpret_cast<const uint4*>(src);
    uint4* d = reinterpret_cast<uint4*>(dst);
    d[0] = s[0];
    d[1] = s[1];
}

// Exclusive position of this thread's flag among the workgroup's set flags, and the workgroup's count.  All BS threads call it;
// s_wave holds BS / 64 ints of LDS.
template <int BS>
__device__ __forceinline__ int psl_wg_compact(bool flag, int* s_wave, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint64_t b = __ballot(flag);
    const uint64_t below = lane ? (b & (~0ull >> (64 - lane))) : 0ull;
    if (lane == 0) s_wave[wave] = __popcll(b);
    __syncthreads();
    int off = 0, tot = 0;
    for (int w = 0; w < BS / 64; ++w) {
        const int c = s_wave[w];
        off += w < wave ? c : 0;
        tot += c;
    }
    __syncthreads();  // s_wave is reused by the next round
    *total = tot;
    return off + __popcll(below);
}

#endif
