// Shared by pslfe_kf.hip, pslfe_match.hip, pslfe_assoc.hip and pslfe_kf_line.hip: the bodies of the one-keyframe line kernels that the
// keyframe-set twins of pslfe_kf_line.hip run too.  Product code.
//   LSDmatcher::Fuse search + KeyFrame::GetLinesInArea   add_src/LSDmatcher.cpp:933-958, src/KeyFrame.cc:857-891
//   knnMatch(k = 2) of LSDmatcher::FrameBFMatch          add_src/LSDmatcher.cpp:492-502
//   lineDescriptorMAD + the three gates                  add_src/LSDmatcher.cpp:503-515, 660-685
#ifndef PSL_KF_LINE_KERNELS_H
#define PSL_KF_LINE_KERNELS_H

#include "match_kernels.h"

// normalised direction startPoint - endPoint of a keyline, as GetLinesInArea forms it (src/KeyFrame.cc:874-877)
__device__ __forceinline__ float2 psl_keyline_dir(const PslKeyLine& kl) {
    const float dx = PSL_FSUB(kl.startPointX, kl.endPointX), dy = PSL_FSUB(kl.startPointY, kl.endPointY);
    const float n = sqrtf(PSL_FADD(PSL_FMUL(dx, dx), PSL_FMUL(dy, dy)));
    return make_float2(PSL_FDIV(dx, n), PSL_FDIV(dy, n));
}

// The keylines of one keyframe as the Fuse search reads them: straight from the caller's arrays ...
struct LineFuseGlobal {
    const PslKeyLine* kls;
    const uint32_t* desc;
    __device__ __forceinline__ float2 pt(int k) const { return make_float2(kls[k].pt_x, kls[k].pt_y); }
    __device__ __forceinline__ float2 dir(int k) const { return psl_keyline_dir(kls[k]); }
    __device__ __forceinline__ int octave(int k) const { return kls[k].octave; }
    __device__ __forceinline__ int hamming(const uint32_t (&qd)[8], int k) const { return psl_hamming256(qd, desc + (size_t)k * 8); }
};
// ... or staged in LDS once per workgroup: pt and the normalised direction (the same sqrtf and divisions, done once per keyline
// instead of once per (map line, keyline)), the octave, the descriptor rows
struct LineFuseLds {
    const float4* geo;   // pt.x pt.y dir.x dir.y
    const int* oct;
    const uint4* desc;   // two per keyline
    __device__ __forceinline__ float2 pt(int k) const { const float4 g = geo[k]; return make_float2(g.x, g.y); }
    __device__ __forceinline__ float2 dir(int k) const { const float4 g = geo[k]; return make_float2(g.z, g.w); }
    __device__ __forceinline__ int octave(int k) const { return oct[k]; }
    __device__ __forceinline__ int hamming(const uint32_t (&qd)[8], int k) const { return psl_hamming256(qd, desc[2 * k], desc[2 * k + 1]); }
};

// LSDmatcher::Fuse search of one projected map line by one wave: KeyFrame::GetLinesInArea is a linear scan of the keyframe's n
// keylines; a keyline without a descriptor row (k >= ndesc) is skipped.  Lane 0 writes *best_idx / *best_dist.
template <typename Src>
__device__ __forceinline__ void psl_line_fuse_row(const Src& S, int n, int ndesc, const PslLineFuseQuery& q, const uint8_t* __restrict__ qdesc,
                                                  int lane, int* __restrict__ best_idx, int* __restrict__ best_dist) {
    if (!(q.radius >= 0)) {
        if (lane == 0) { *best_idx = -1; *best_dist = 256; }
        return;
    }
    const uint32_t* QD = reinterpret_cast<const uint32_t*>(qdesc);
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) qd[k] = QD[k];
    float d1x = PSL_FSUB(q.x1, q.x2), d1y = PSL_FSUB(q.y1, q.y2);
    const float n1 = sqrtf(PSL_FADD(PSL_FMUL(d1x, d1x), PSL_FMUL(d1y, d1y)));
    d1x = PSL_FDIV(d1x, n1);
    d1y = PSL_FDIV(d1y, n1);
    const double mx = PSL_DMUL(0.5, (double)PSL_FADD(q.x1, q.x2)), my = PSL_DMUL(0.5, (double)PSL_FADD(q.y1, q.y2));
    const float rr = PSL_FMUL(q.radius, q.radius);
    uint32_t best = PSL_KEY_INF;
    for (int k = lane; k < n; k += 64) {
        const float2 pt = S.pt(k);
        const double ddx = PSL_DSUB(mx, (double)pt.x), ddy = PSL_DSUB(my, (double)pt.y);
        const float distance = (float)PSL_DADD(PSL_DMUL(ddx, ddx), PSL_DMUL(ddy, ddy));
        if (distance > rr) continue;
        const float2 d2 = S.dir(k);
        const float cs = __builtin_fabsf(PSL_FADD(PSL_FMUL(d1x, d2.x), PSL_FMUL(d1y, d2.y)));
        if (cs < 0.998f) continue;
        const int octave = S.octave(k);
        if (octave < q.level - 1 || octave > q.level) continue;
        if (k >= ndesc) continue;
        best = min(best, ((uint32_t)S.hamming(qd, k) << 16) | (uint32_t)k);
    }
    best = psl_wave_min_u32(best);
    if (lane == 0) {
        // bestDist starts at 256 and moves on dist < bestDist only (:933-958): a candidate at distance 256 is no candidate
        const bool none = best >= (256u << 16);
        *best_idx = none ? -1 : (int)(best & 0xffffu);
        *best_dist = none ? 256 : (int)(best >> 16);
    }
}

// The two nearest rows of t (nt < 2^20 rows) to query row q, by one wave; lane 0 writes idx[0..1] / dist[0..1] (-1 / INT_MAX when
// there is no such row).
__device__ __forceinline__ void psl_knn2_row(const uint8_t* __restrict__ q, const uint8_t* __restrict__ t, int nt, int lane,
                                             int* __restrict__ idx, int* __restrict__ dist) {
    uint32_t qd[8];
    const uint32_t* Q = reinterpret_cast<const uint32_t*>(q);
#pragma unroll
    for (int k = 0; k < 8; ++k) qd[k] = Q[k];
    const uint32_t* T = reinterpret_cast<const uint32_t*>(t);
    uint32_t k1 = 0xffffffffu, k2 = 0xffffffffu;
    for (int j = lane; j < nt; j += 64) {
        const uint32_t key = ((uint32_t)psl_hamming256(qd, T + (size_t)j * 8) << 20) | (uint32_t)j;  // nt < 2^20
        if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
    }
    psl_wave_min2(k1, k2);
    if (lane == 0) {
        idx[0] = k1 == 0xffffffffu ? -1 : (int)(k1 & 0xfffff);
        dist[0] = k1 == 0xffffffffu ? 0x7fffffff : (int)(k1 >> 20);
        idx[1] = k2 == 0xffffffffu ? -1 : (int)(k2 & 0xfffff);
        dist[1] = k2 == 0xffffffffu ? 0x7fffffff : (int)(k2 >> 20);
    }
}

// FrameBFMatch after knnMatch, by one workgroup of 256 threads: MAD of (d1 - d0), then the three gates (:503-515).  scratch: 2 * n1
// floats; s_med: one float of LDS.
__device__ __forceinline__ void psl_frame_bf_gate(const int* __restrict__ knn_idx, const int* __restrict__ knn_dist, int n1, float nnratio,
                                                  float TH, float* __restrict__ scratch, int* __restrict__ lineMatches, float* s_med) {
    float* d12 = scratch;        // [n1]
    float* dev = scratch + n1;   // [n1]
    const int tid = threadIdx.x;
    for (int i = tid; i < n1; i += 256) d12[i] = PSL_FSUB((float)knn_dist[2 * i + 1], (float)knn_dist[2 * i]);
    __syncthreads();
    for (int i = tid; i < n1; i += 256) {  // the element of rank n1/2 of the sorted values
        const float v = d12[i];
        int r = 0;
        for (int j = 0; j < n1; ++j) { const float u = d12[j]; r += (u < v) || (u == v && j < i); }
        if (r == n1 / 2) *s_med = v;
    }
    __syncthreads();
    const double med = (double)*s_med;
    for (int i = tid; i < n1; i += 256) dev[i] = __builtin_fabsf((float)PSL_DSUB((double)d12[i], med));
    __syncthreads();
    for (int i = tid; i < n1; i += 256) {
        const float v = dev[i];
        int r = 0;
        for (int j = 0; j < n1; ++j) { const float u = dev[j]; r += (u < v) || (u == v && j < i); }
        if (r == n1 / 2) *s_med = v;
    }
    __syncthreads();
    const double nn12_th = PSL_DMUL(PSL_DMUL(1.4826, (double)*s_med), 0.5);
    for (int i = tid; i < n1; i += 256) {
        const float a = (float)knn_dist[2 * i], b = (float)knn_dist[2 * i + 1];
        lineMatches[i] = ((double)PSL_FSUB(b, a) > nn12_th && a < TH && a < PSL_FMUL(nnratio, b)) ? knn_idx[2 * i] : -1;
    }
}

#endif
