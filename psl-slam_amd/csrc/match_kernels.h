// The matcher primitives of every ORB search on the device.  Product code.
// Users: pslfe_match.hip (Tracking searches, SearchByBoW), pslfe_kf.hip (Fuse, SearchBySim3, SearchForTriangulation),
// pslfe_mono.hip (SearchForInitialization), pslfe_loop.hip (loop-closing searches), pslfe_stereo.hip / stereo_kernels.h
// (ComputeStereoMatches), pslfe_project.hip (frame store only), pslfe_bow.hip and pslfe_linematch.hip (Hamming and wave helpers).
// What it offers:
//   frame store       FrameMeta / FrameStore / FrameView: keypoints bucketed on the 64x48 grid of include/Frame.h:45-46 as CSR runs
//   wave helpers      psl_wave_min_u32, psl_wave_sum, psl_merge2 / psl_wave_min2 (two smallest keys), psl_wave_sort, psl_topk_merge
//   Hamming           psl_hamming256: query in registers against two uint4 halves, or against a pointer
//   rotation check    psl_rot_bin, psl_three_maxima (ComputeThreeMaxima), psl_rot_keep
//   window            psl_grid_cols / psl_window_cols (GetFeaturesInArea as column runs), psl_window_pos
//   candidate key     psl_window_key over a candidate accessor (FrameCands here; a kernel with a staged frame brings its own)
// A new search starts from these and keeps for itself only what is its own: its gates and its histogram fill loop.
#ifndef PSL_MATCH_KERNELS_H
#define PSL_MATCH_KERNELS_H
#include <vector>

#include "pslfe_internal.h"
#include "psl_device_math.h"

#define PSL_GRID_COLS 64
#define PSL_GRID_ROWS 48
#define PSL_GRID_CELLS (PSL_GRID_COLS * PSL_GRID_ROWS)
#define PSL_QMAX 4096      // most queries / keypoints one workgroup handles
#define PSL_TH_HIGH 100    // ORBmatcher::TH_HIGH src/ORBmatcher.cc:37
#define PSL_TH_LOW 50      // ORBmatcher::TH_LOW :38, LSDmatcher::TH_LOW
#define PSL_HISTO 30       // ORBmatcher::HISTO_LENGTH :39

struct FrameMeta {
    int n;
    float minX, minY, invW, invH;
};

struct FrameStore {  // slot s lives at [s * cap] of every array
    PslKeyPoint* kps;
    uint8_t* desc;
    float* uright;
    uint16_t* cellof;
    int* gstart;  // [slot][PSL_GRID_CELLS + 1]
    int* gidx;    // [slot][cap]
    FrameMeta* meta;
    int cap;
};


// 256-bit Hamming distance of a query held in registers and a candidate given as its two 128-bit halves
__device__ __forceinline__ int psl_hamming256(const uint32_t (&q)[8], const uint4 d0, const uint4 d1) {
    return __popc(q[0] ^ d0.x) + __popc(q[1] ^ d0.y) + __popc(q[2] ^ d0.z) + __popc(q[3] ^ d0.w) + __popc(q[4] ^ d1.x) +
           __popc(q[5] ^ d1.y) + __popc(q[6] ^ d1.z) + __popc(q[7] ^ d1.w);
}

__device__ __forceinline__ int psl_hamming256(const uint32_t (&q)[8], const uint32_t* __restrict__ d) {  // d: 16-byte aligned
    return psl_hamming256(q, *reinterpret_cast<const uint4*>(d), *reinterpret_cast<const uint4*>(d + 4));
}

__device__ __forceinline__ uint32_t psl_wave_min_u32(uint32_t v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, (uint32_t)__shfl_xor((int)v, o));
    return v;
}

__device__ __forceinline__ int psl_wave_sum(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// exclusive scan of one int per thread over a workgroup of 256 threads; *total = the sum.  s_w: 4 ints of LDS.  Called by every thread.
__device__ __forceinline__ int psl_block_scan_256(int v, int* s_w, int* total) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int incl = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    __syncthreads();   // the previous call's reads of s_w
    if (lane == 63) s_w[wave] = incl;
    __syncthreads();
    int base = 0, sum = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) { if (w < wave) base += s_w[w]; sum += s_w[w]; }
    *total = sum;
    return base + incl - v;
}

// (k1, k2) <- the two smallest of {k1, k2, o1, o2}, given k1 <= k2 and o1 <= o2
__device__ __forceinline__ void psl_merge2(uint32_t& k1, uint32_t& k2, uint32_t o1, uint32_t o2) {
    const uint32_t lo = min(k1, o1), hi = max(k1, o1);
    k2 = min(hi, min(k2, o2));
    k1 = lo;
}

// every lane's two smallest keys (k1 <= k2) -> the two smallest of the wave, in all lanes
__device__ __forceinline__ void psl_wave_min2(uint32_t& k1, uint32_t& k2) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) psl_merge2(k1, k2, __shfl_xor(k1, o), __shfl_xor(k2, o));
}

// Rotation consistency of the ORBmatcher searches: bin of angle1 - angle2 in the HISTO_LENGTH histogram (src/ORBmatcher.cc:607-612)
__device__ __forceinline__ int psl_rot_bin(float a1, float a2) {
    float rot = PSL_FSUB(a1, a2);
    if (rot < 0.0f) rot = PSL_FADD(rot, 360.0f);
    int bin = (int)__builtin_roundf(PSL_FMUL(rot, 1.0f / PSL_HISTO));
    if (bin == PSL_HISTO) bin = 0;
    return bin < 0 ? 0 : (bin >= PSL_HISTO ? PSL_HISTO - 1 : bin);
}

// ORBmatcher::ComputeThreeMaxima (:1601-1645) of hist[PSL_HISTO] into ind[3]; one thread, on LDS
__device__ __forceinline__ void psl_three_maxima(const int* hist, int* ind) {
    int max1 = 0, max2 = 0, max3 = 0, ind1 = -1, ind2 = -1, ind3 = -1;
    for (int i = 0; i < PSL_HISTO; ++i) {
        const int sz = hist[i];
        if (sz > max1) { max3 = max2; max2 = max1; max1 = sz; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (sz > max2) { max3 = max2; max2 = sz; ind3 = ind2; ind2 = i; }
        else if (sz > max3) { max3 = sz; ind3 = i; }
    }
    if ((float)max2 < PSL_FMUL(0.1f, (float)max1)) { ind2 = -1; ind3 = -1; }
    else if ((float)max3 < PSL_FMUL(0.1f, (float)max1)) { ind3 = -1; }
    ind[0] = ind1; ind[1] = ind2; ind[2] = ind3;
}

__device__ __forceinline__ bool psl_rot_keep(int bin, const int* ind) { return bin == ind[0] || bin == ind[1] || bin == ind[2]; }

struct MatchArgs {
    FrameStore S;
    int slot0;
    const PslProjQuery* q;
    const uint8_t* qdesc;
    const int* nq_arr;
    int nq_single, qstride;
    const uint8_t* taken;
    int check_ori;
    float nnratio;
    int* match;
    int* assigned;
    int* nmatches;
    uint32_t* topk;   // [pair][qstride][PSL_TOPK]: the smallest keys (dist << 16 | CSR position) of every query, ascending
    uint8_t* more;    // [pair][qstride]: the query has more than PSL_TOPK gated candidates
    int th;           // descriptor-distance gate of the decision: TH_HIGH, ORBdist or TH_LOW
    int no_stereo;    // skip the mvuRight gate (SearchByProjection(cur,KF), SearchByBoW)
    const int* fidx;  // != NULL: candidates of a query are the run [min_level, min_level + max_level) of this index list
                      // (the frame's DBoW2 FeatureVector flattened in node order) instead of a grid window
};

#define PSL_KEY_INF 0xffffffffu

__device__ __forceinline__ void psl_top4_insert(uint32_t (&t)[4], uint32_t key) {
    if (key < t[3]) {
        t[3] = key;
        if (t[3] < t[2]) { const uint32_t u = t[2]; t[2] = t[3]; t[3] = u; }
        if (t[2] < t[1]) { const uint32_t u = t[1]; t[1] = t[2]; t[2] = u; }
        if (t[1] < t[0]) { const uint32_t u = t[0]; t[0] = t[1]; t[1] = u; }
    }
}

struct FrameView {
    const PslKeyPoint* kps;
    const uint32_t* desc;
    const float* uright;
    const int* gstart;
    const int* gidx;
    FrameMeta M;
    int n;
};

__device__ __forceinline__ FrameView psl_frame_view(const FrameStore& S, int slot) {
    FrameView V;
    V.M = S.meta[slot];
    V.kps = S.kps + (size_t)slot * S.cap;
    V.desc = reinterpret_cast<const uint32_t*>(S.desc + (size_t)slot * S.cap * 32);
    V.uright = S.uright + (size_t)slot * S.cap;
    V.gstart = S.gstart + (size_t)slot * (PSL_GRID_CELLS + 1);
    V.gidx = S.gidx + (size_t)slot * S.cap;
    V.n = V.M.n < PSL_QMAX ? V.M.n : PSL_QMAX;
    return V;
}

// GetFeaturesInArea window of one query (src/Frame.cc:985-1038), one wave per query.  Grid column ix of the window
// (cells nMinCellY..nMaxCellY) is one contiguous CSR run; lane l fetches the run of column nMinCellX + l and a wave
// scan flattens the runs into candidate numbers 0..T-1 in the reference's visiting order.  Lane l then evaluates
// candidates l, l + 64, ...: every candidate costs the same three dependent fetches (run bounds -> keypoint index
// -> keypoint, descriptor, gates) no matter how many share its column, and all lanes work even for narrow windows.
struct WindowCols {
    int start, excl, incl, T;
    bool checkLevels;
};

// The window of (u, v, r) on the CSR grid `gstart` (a frame's, a reduced one, or a copy in LDS).  Called by all 64 lanes.
__device__ __forceinline__ WindowCols psl_grid_cols(const int* gstart, const FrameMeta& M, float u, float v, float r) {
    const int lane = threadIdx.x & 63;
    const int minCX = max(0, (int)__builtin_floorf(PSL_FMUL(PSL_FSUB(PSL_FSUB(u, M.minX), r), M.invW)));
    const int maxCX = min(PSL_GRID_COLS - 1, (int)__builtin_ceilf(PSL_FMUL(PSL_FADD(PSL_FSUB(u, M.minX), r), M.invW)));
    const int minCY = max(0, (int)__builtin_floorf(PSL_FMUL(PSL_FSUB(PSL_FSUB(v, M.minY), r), M.invH)));
    const int maxCY = min(PSL_GRID_ROWS - 1, (int)__builtin_ceilf(PSL_FMUL(PSL_FADD(PSL_FSUB(v, M.minY), r), M.invH)));
    const bool window = minCX < PSL_GRID_COLS && maxCX >= 0 && minCY < PSL_GRID_ROWS && maxCY >= 0;
    WindowCols W;
    W.start = 0;
    int len = 0;
    if (window && minCX + lane <= maxCX) {
        const int ix = minCX + lane;
        W.start = gstart[ix * PSL_GRID_ROWS + minCY];
        len = gstart[ix * PSL_GRID_ROWS + maxCY + 1] - W.start;
    }
    int incl = len;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int t = __shfl_up(incl, o); if (lane >= o) incl += t; }
    W.incl = incl;
    W.excl = incl - len;
    W.T = __shfl(incl, 63);
    W.checkLevels = false;
    return W;
}

__device__ __forceinline__ WindowCols psl_window_cols(const FrameView& V, const PslProjQuery& q, const int* fidx) {
    if (fidx) {  // one run: the frame's features under the query's vocabulary node
        const int lane = threadIdx.x & 63;
        WindowCols W;
        W.start = lane == 0 ? q.min_level : 0;
        const int len = lane == 0 ? (q.max_level > 0 ? q.max_level : 0) : 0;
        W.incl = len > 0 ? len : 0;
        W.incl = __shfl(W.incl, 0);  // inclusive counts: every lane >= 0 holds the total
        W.excl = lane == 0 ? 0 : W.incl;
        W.T = W.incl;
        W.checkLevels = false;
        return W;
    }
    WindowCols W = psl_grid_cols(V.gstart, V.M, q.u, q.v, q.radius);
    W.checkLevels = (q.min_level > 0) || (q.max_level >= 0);
    return W;
}

// CSR position of candidate number j of the window, -1 if j >= T.  Called by all 64 lanes (shuffles inside).
__device__ __forceinline__ int psl_window_pos(const WindowCols& W, int j) {
    int c = 0;  // number of columns whose inclusive count is <= j == the column of candidate j
#pragma unroll
    for (int step = 32; step > 0; step >>= 1) {
        const int v = __shfl(W.incl, c + step - 1);
        if (v <= j) c += step;
    }
    c = c < 63 ? c : 63;
    const int cs = __shfl(W.start, c), ce = __shfl(W.excl, c);
    return j < W.T ? cs + (j - ce) : -1;
}

// What a window search fetches of the candidate at CSR position p, from the frame store: the keypoint index and, by index, the
// keypoint's fields.  `windowed` is false where the candidates are a feature-vector run (fidx) and not a grid window.
struct FrameCands {
    const FrameView& V;
    const int* fidx;
    __device__ bool windowed() const { return !fidx; }
    __device__ int index(int p) const { return fidx ? fidx[p] : V.gidx[p]; }
    __device__ bool inside(int i2) const { return i2 >= 0 && i2 < V.n; }
    __device__ float2 xy(int i2) const { return *reinterpret_cast<const float2*>(&V.kps[i2].x); }
    __device__ int octave(int i2) const { return V.kps[i2].octave; }
    __device__ float uright(int i2) const { return V.uright[i2]; }
    __device__ uint4 desc0(int i2) const { return *reinterpret_cast<const uint4*>(V.desc + (size_t)i2 * 8); }
    __device__ uint4 desc1(int i2) const { return *reinterpret_cast<const uint4*>(V.desc + (size_t)i2 * 8 + 4); }
};

// Key (distance << 16 | CSR position) of candidate number j, PSL_KEY_INF if j >= T or a gate rejects it: level band,
// window, stereo (:1405-1411), taken initially (:1401-1403), taken by an earlier query of this call (blocker != NULL), distance 256.
// Called by all 64 lanes (shuffles inside).
template <typename Cands>
__device__ __forceinline__ uint32_t psl_window_key(const Cands& C, const PslProjQuery& q, const uint32_t (&qd)[8], const uint8_t* taken,
                                                   const int* blocker, int qi, const WindowCols& W, int j, int no_stereo) {
    const int p = psl_window_pos(W, j);
    uint32_t key = PSL_KEY_INF;
    if (p >= 0) {
        const float r = q.radius;
        const int i2 = C.index(p);
        const float2 xy = C.xy(i2);
        const int octave = C.octave(i2);
        const float ur = C.uright(i2);
        const uint4 d0 = C.desc0(i2), d1 = C.desc1(i2);
        bool ok = C.inside(i2);
        if (C.windowed()) {
            if (W.checkLevels) ok = ok && !(octave < q.min_level) && !(q.max_level >= 0 && octave > q.max_level);
            ok = ok && (__builtin_fabsf(PSL_FSUB(xy.x, q.u)) < r && __builtin_fabsf(PSL_FSUB(xy.y, q.v)) < r);
        }
        if (taken) ok = ok && !taken[i2];
        if (blocker) ok = ok && !(blocker[i2] < qi);
        if (!no_stereo) ok = ok && !(ur > 0 && __builtin_fabsf(PSL_FSUB(q.ur, ur)) > r);
        const int dist = psl_hamming256(qd, d0, d1);
        // dist < 256: every search starts from bestDist = bestDist2 = 256 and compares with a strict < (src/ORBmatcher.cc:76-78, :102,
        // :110, :1397, :1419, :1535, :1548), so the complement of the query is never the best nor the second best
        if (ok && dist < 256) key = ((uint32_t)dist << 16) | (uint32_t)p;
    }
    return key;
}

// Ascending bitonic sort of one 32-bit key per lane across the wave.
__device__ __forceinline__ uint32_t psl_wave_sort(uint32_t v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
        for (int j = k >> 1; j > 0; j >>= 1) {
            const uint32_t o = __shfl_xor(v, j);
            const bool up = (lane & k) == 0, lower = (lane & j) == 0;
            v = (up == lower) ? min(v, o) : max(v, o);
        }
    }
    return v;
}

// One round of the running top-K of pass 1.  `best`: the K smallest keys so far in lanes 0..K-1, ascending (unused in the first
// round); `key`: this round's key of every lane.  Returns the new running list, again in lanes 0..K-1.
template <int K>
__device__ __forceinline__ uint32_t psl_topk_merge(uint32_t best, uint32_t key, bool first_round) {
    const int lane = threadIdx.x & 63;
    key = psl_wave_sort(key);
    if (!first_round) {  // merge this round's smallest with the running ones
        const uint32_t o = __shfl(key, (lane - K) & 63);
        key = psl_wave_sort(lane < K ? best : (lane < 2 * K ? o : PSL_KEY_INF));
    }
    return key;
}

struct pslfe_frame {
    pslfe_ctx* ctx = nullptr;
    int cap = 0, max_frames = 0;
    FrameStore S = {};
    // scratch for the host-pointer entry points
    PslProjQuery* d_q = nullptr;
    uint8_t* d_qdesc = nullptr;
    uint8_t* d_taken = nullptr;
    int* d_match = nullptr;
    int* d_assigned = nullptr;
    int* d_nm = nullptr;
    uint32_t* d_topk = nullptr;  // [max_frames][cap][PSL_TOPK]
    uint8_t* d_more = nullptr;   // [max_frames][cap]
    uint32_t* d_topk1 = nullptr; // [PSL_QMAX][PSL_TOPK] for the host-pointer entry points
    uint8_t* d_more1 = nullptr;
    int* d_fidx = nullptr;       // [cap] the frame's FeatureVector (SearchByBoW, host-pointer entry point)
    float* d_depth = nullptr;    // [max_frames][cap] mvDepth (RGB-D post-processing)
    float* d_bounds = nullptr;   // [4] scratch for k_image_bounds
    // stereo (pslfe_stereo.hip), allocated on the first stereo call: taps [max_frames][cap], right keypoints binned by row
    int32_t* d_st_idx = nullptr;
    int32_t* d_st_sad = nullptr;
    int* d_st_rowstart = nullptr;     // [pairs][rows + 1]
    uint16_t* d_st_rowidx = nullptr;  // [pairs][right capacity]
    size_t st_rowstart_cap = 0, st_rowidx_cap = 0;
    PslDeviceBuffers mem;        // owns every device buffer above
    std::vector<char> slot_set;
    std::vector<char> slot_depth;  // the slot's mvDepth was set (pslfe_frame_set_rgbd / _set_from_orb_rgbd / _set_from_orb_stereo)
    std::vector<char> slot_stereo; // the slot was set by pslfe_frame_set_from_orb_stereo (its taps are valid)
};

struct pslfe_kf {   // pslfe_kf.hip, pslfe_loop.hip: the per-call buffers come from the context's scratch arena
    pslfe_ctx* ctx = nullptr;
    int upkeep_sum = PSLFE_UPKEEP_SUM_WALK;   // pslfe_map_upkeep.hip: the layout of the run-order sums (pslfe_kf_set_upkeep_sum)
};

// pslfe_match.hip, for pslfe_stereo.hip: frames of an extractor's result arrays (pointers at the first frame) -> slots
// slot0.., and the constructor's tail on those slots (bounds of a cols x rows image, UndistortKeyPoints, grid)
extern "C" int psl_frame_import(pslfe_frame* f, int slot0, const PslKeyPoint* okps, const uint8_t* odesc, const int* ocounts, int ocap,
                                int nframes);
extern "C" int psl_frame_finish_stereo(pslfe_frame* f, int slot0, int nslots, int cols, int rows, const PslCamera* cam);

#endif
