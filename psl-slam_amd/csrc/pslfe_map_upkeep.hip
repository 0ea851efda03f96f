// libpslfe: the geometry half of the map refresh of LocalMapping / LoopClosing, for every map point or map line of a call.  Product code.
// Reference behaviour reproduced:
//   MapPoint::UpdateNormalAndDepth        src/MapPoint.cc:330-371         (M map points)
//   MapLine::UpdateAverageDir             add_src/MapLine.cpp:320-367     (M map lines)
//   KeyFrame::ComputeSceneMedianDepth     src/KeyFrame.cc:749-779         (K keyframes)
// Conventions: include/pslfe.h above pslfe_kf_update_normal_and_depth; primitives: proj_kernels.h (the double norm, the affine row, the
// half-sum of the line projections) and the single-operation macros of psl_device_math.h.
//
// Refresh: the terms of a run are independent, their sum is ordered.  Two layouts of the same arithmetic (pslfe_kf_set_upkeep_sum):
//   walk   one thread per row walks its run: index, centre, term, add.  Rows of different run lengths diverge and every read is a gather.
//   tiled  a workgroup owns PSL_UPK_BS consecutive rows, whose runs are one stretch of obs_kf.  The stretch is taken in tiles: one lane per
//          observation (coalesced index reads; the owner row by bisection of the staged offsets) writes the term to LDS, then the thread
//          that owns a row adds the tile's terms of its run in run order to the sum it keeps in registers.
// Both give the same bytes (tests/test_map_upkeep_gpu.py).  The walk is the default; the two have not been measured against each other
// (DESIGN.md §5.0j).  The tiled layout forms the terms of skipped rows too, so obs_kf must be in range for every run.
// Median depth: one workgroup per keyframe; the depth of rank (n-1)/q is found by a four-pass radix selection on the order-preserving
// key of the float, with the 256 counters of a pass in LDS.  The depths are recomputed from x in every pass (12 B per point from L2).
#include <string.h>

#include "pslfe_internal.h"
#include "psl_device_math.h"

#include "match_kernels.h"
#include "proj_kernels.h"

#define PSL_UPK_BS 256
#define PSL_UPK_TILE 2048   // terms of one tile in LDS: 24 KB of float triples, 48 KB of double triples

static_assert(sizeof(PslMapPointGeom) == 32 && sizeof(PslMapLineGeom) == 80 && sizeof(PslPose) == 48, "map upkeep PODs");

struct UpkeepArgs {
    void* rows;                // PslMapPointGeom / PslMapLineGeom [M], updated in place
    int M;
    const int32_t* obs_off;    // [M + 1]
    const int32_t* obs_kf;     // [obs_off[M]]
    const float* centres;      // [nkf][3]
    const int32_t* ref_kf;     // [M]
    const int32_t* ref_level;  // [M]
    const uint8_t* skip;       // [M] or NULL
    float scale[PSLFE_MAX_LEVELS];
    int nlevels;
};

// mfMaxDistance = dist*levelScaleFactor; mfMinDistance = mfMaxDistance/mvScaleFactors[nLevels-1] (src/MapPoint.cc:367-368)
__device__ __forceinline__ void psl_upk_range(const UpkeepArgs& A, int i, float dist, float* min_dist, float* max_dist) {
    *max_dist = PSL_FMUL(dist, A.scale[A.ref_level[i]]);
    *min_dist = PSL_FDIV(*max_dist, A.scale[A.nlevels - 1]);
}

// MapPoint::UpdateNormalAndDepth: float terms, a float sum
struct UpkPoint {
    typedef float T;
    struct Pos { float p[3]; };
    static __device__ __forceinline__ Pos load(const void* rows, int i) {
        const float4 a = reinterpret_cast<const float4*>(rows)[2 * (size_t)i];
        Pos P = {{a.x, a.y, a.z}};
        return P;
    }
    // normali/cv::norm(normali) (:354-355): Mat / double scales by the reciprocal, rounded to the Mat's float
    static __device__ __forceinline__ void term(const Pos& P, const float* ow, T* out) {
        const float n0 = PSL_FSUB(P.p[0], ow[0]), n1 = PSL_FSUB(P.p[1], ow[1]), n2 = PSL_FSUB(P.p[2], ow[2]);
        const float t = (float)PSL_DDIV(1.0, psl_norm3_d(n0, n1, n2));
        out[0] = PSL_FMUL(n0, t); out[1] = PSL_FMUL(n1, t); out[2] = PSL_FMUL(n2, t);
    }
    static __device__ __forceinline__ T add(T a, T b) { return PSL_FADD(a, b); }
    // normal/n, the distance to the reference keyframe and its range (:359-369); x, y, z are not written
    static __device__ __forceinline__ void finish(const UpkeepArgs& A, int i, const Pos& P, const T* sum, int n) {
        const float t = (float)PSL_DDIV(1.0, (double)n);
        const float* ow = A.centres + 3 * (size_t)A.ref_kf[i];
        const float dist = psl_norm3(PSL_FSUB(P.p[0], ow[0]), PSL_FSUB(P.p[1], ow[1]), PSL_FSUB(P.p[2], ow[2]));
        float min_dist, max_dist;
        psl_upk_range(A, i, dist, &min_dist, &max_dist);
        float* row = reinterpret_cast<float*>(A.rows) + 8 * (size_t)i;
        row[3] = PSL_FMUL(sum[0], t);
        reinterpret_cast<float4*>(row)[1] = make_float4(PSL_FMUL(sum[1], t), PSL_FMUL(sum[2], t), min_dist, max_dist);
    }
};

// MapLine::UpdateAverageDir: Eigen double terms, a double sum; the depth range through float Mats
struct UpkLine {
    typedef double T;
    struct Pos { double sp[3], ep[3]; };
    static __device__ __forceinline__ Pos load(const void* rows, int i) {
        const double2* G = reinterpret_cast<const double2*>(rows) + 5 * (size_t)i;
        const double2 g0 = G[0], g1 = G[1], g2 = G[2];   // sp0 sp1 | sp2 ep0 | ep1 ep2
        Pos P = {{g0.x, g0.y, g1.x}, {g1.y, g2.x, g2.y}};
        return P;
    }
    // middlePos = 0.5*(head+tail); normali = middlePos - OWi; normali/normali.norm() (:345-347): a division per component
    static __device__ __forceinline__ void term(const Pos& P, const float* ow, T* out) {
        double n[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) n[c] = PSL_DSUB(PSL_DMUL(0.5, PSL_DADD(P.sp[c], P.ep[c])), (double)ow[c]);
        double s = PSL_DMUL(n[0], n[0]);
        s = PSL_DADD(s, PSL_DMUL(n[1], n[1]));
        s = PSL_DADD(s, PSL_DMUL(n[2], n[2]));
        const double nrm = PSL_DSQRT(s);
#pragma unroll
        for (int c = 0; c < 3; ++c) out[c] = PSL_DDIV(n[c], nrm);
    }
    static __device__ __forceinline__ T add(T a, T b) { return PSL_DADD(a, b); }
    // normal/n; SP, EP as float Mats, MP = 0.5*(SP+EP), CM = MP - Ow, dist = cv::norm(CM) (:351-365)
    static __device__ __forceinline__ void finish(const UpkeepArgs& A, int i, const Pos& P, const T* sum, int n) {
        const float* ow = A.centres + 3 * (size_t)A.ref_kf[i];
        float CM[3];
#pragma unroll
        for (int c = 0; c < 3; ++c) CM[c] = PSL_FSUB(psl_half_sum((float)P.sp[c], (float)P.ep[c]), ow[c]);
        const float dist = psl_norm3(CM[0], CM[1], CM[2]);
        float min_dist, max_dist;
        psl_upk_range(A, i, dist, &min_dist, &max_dist);
        const double dn = (double)n;
        double2* G = reinterpret_cast<double2*>(A.rows) + 5 * (size_t)i;
        G[3] = make_double2(PSL_DDIV(sum[0], dn), PSL_DDIV(sum[1], dn));
        G[4] = make_double2(PSL_DDIV(sum[2], dn), __hiloint2double(__float_as_int(max_dist), __float_as_int(min_dist)));
    }
};

// a row with an empty run or a skip byte keeps its bytes: the early returns of :338-346
__device__ __forceinline__ bool psl_upk_live(const UpkeepArgs& A, int i, int b, int e) { return e > b && !(A.skip && A.skip[i]); }

template <class U>
__global__ __launch_bounds__(PSL_UPK_BS) void k_upkeep_walk(UpkeepArgs A) {
    const int i = blockIdx.x * PSL_UPK_BS + threadIdx.x;
    if (i >= A.M) return;
    const int b = A.obs_off[i], e = A.obs_off[i + 1];
    if (!psl_upk_live(A, i, b, e)) return;
    const typename U::Pos P = U::load(A.rows, i);
    typename U::T sum[3] = {0, 0, 0};
    for (int o = b; o < e; ++o) {
        typename U::T t[3];
        U::term(P, A.centres + 3 * (size_t)A.obs_kf[o], t);
#pragma unroll
        for (int c = 0; c < 3; ++c) sum[c] = U::add(sum[c], t[c]);
    }
    U::finish(A, i, P, sum, e - b);
}

template <class U>
__global__ __launch_bounds__(PSL_UPK_BS) void k_upkeep_tiled(UpkeepArgs A) {
    __shared__ int s_off[PSL_UPK_BS + 1];
    __shared__ typename U::T s_term[3][PSL_UPK_TILE];
    const int tid = threadIdx.x, p0 = blockIdx.x * PSL_UPK_BS;
    const int np = min(PSL_UPK_BS, A.M - p0);   // rows of this workgroup, >= 1
    for (int t = tid; t <= np; t += PSL_UPK_BS) s_off[t] = A.obs_off[p0 + t];
    __syncthreads();
    const int o0 = s_off[0], o1 = s_off[np];
    const int i = p0 + tid;
    int b = 0, e = 0;
    if (tid < np) { b = s_off[tid]; e = s_off[tid + 1]; }
    const bool live = tid < np && psl_upk_live(A, i, b, e);
    typename U::T sum[3] = {0, 0, 0};
    for (int base = o0; base < o1; base += PSL_UPK_TILE) {   // uniform over the workgroup
        const int cnt = min(PSL_UPK_TILE, o1 - base);
        for (int j = tid; j < cnt; j += PSL_UPK_BS) {
            const int o = base + j;
            int lo = 0, hi = np;   // the owner: the last row t with s_off[t] <= o (rows with empty runs in front of it share its offset)
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (s_off[mid] <= o) lo = mid; else hi = mid;
            }
            typename U::T t[3];
            U::term(U::load(A.rows, p0 + lo), A.centres + 3 * (size_t)A.obs_kf[o], t);
#pragma unroll
            for (int c = 0; c < 3; ++c) s_term[c][j] = t[c];
        }
        __syncthreads();
        if (live) {
            const int jb = max(b, base) - base, je = min(e, base + cnt) - base;
            for (int j = jb; j < je; ++j) {
#pragma unroll
                for (int c = 0; c < 3; ++c) sum[c] = U::add(sum[c], s_term[c][j]);
            }
        }
        __syncthreads();   // the next tile overwrites s_term; finish() below overwrites rows, after every term has been formed
    }
    if (live) U::finish(A, i, U::load(A.rows, i), sum, e - b);
}

// ---- KeyFrame::ComputeSceneMedianDepth ---------------------------------------------------------------------------------------------
// the order of the floats as an order of unsigned integers (NaN excluded by precondition)
__device__ __forceinline__ uint32_t psl_float_key(float z) {
    const uint32_t u = __float_as_uint(z);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float psl_key_float(uint32_t k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

__global__ __launch_bounds__(256) void k_scene_median_depth(const PslPose* __restrict__ Tcw, const float* __restrict__ x, const int32_t* __restrict__ off,
                                                            int q, float* __restrict__ depth) {
    __shared__ int s_hist[256];
    __shared__ uint32_t s_prefix;
    __shared__ int s_rank;
    const int k = blockIdx.x, tid = threadIdx.x;
    const int o0 = off[k], n = off[k + 1] - o0;
    if (n <= 0) {   // the reference indexes vDepths[-1 / q] there
        if (tid == 0) depth[k] = -1.0f;
        return;
    }
    const float* T = reinterpret_cast<const float*>(Tcw + k);
    const float r0 = T[6], r1 = T[7], r2 = T[8], tz = T[11];   // Tcw.row(2).colRange(0,3), Tcw.at<float>(2,3)
    if (tid == 0) { s_prefix = 0; s_rank = (n - 1) / q; }
    for (int shift = 24; shift >= 0; shift -= 8) {
        s_hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = s_prefix;
        const uint32_t mask = shift == 24 ? 0u : 0xffffffffu << (shift + 8);
        for (int j = tid; j < n; j += 256) {
            const float* p = x + 3 * ((size_t)o0 + j);
            const uint32_t key = psl_float_key(psl_affine_row(r0, r1, r2, p[0], p[1], p[2], tz));   // float z = Rcw2.dot(x3Dw)+zcw
            if ((key & mask) == prefix) atomicAdd(&s_hist[(key >> shift) & 255], 1);
        }
        __syncthreads();
        if (tid == 0) {   // the byte whose bucket holds the rank among the keys that share the prefix
            int rank = s_rank, bkt = 0;
            while (bkt < 255 && rank >= s_hist[bkt]) rank -= s_hist[bkt++];
            s_prefix = prefix | ((uint32_t)bkt << shift);
            s_rank = rank;
        }
        __syncthreads();
    }
    if (tid == 0) depth[k] = psl_key_float(s_prefix);
}

// ---------------------------------------------------------------------------------------------
namespace {

struct UpkeepHost {   // the arguments of a refresh as the entry points take them
    void* rows; int M;
    const int32_t* obs_off; const int32_t* obs_kf;
    const float* centres; int nkf;
    const int32_t* ref_kf; const int32_t* ref_level;
    const uint8_t* skip;
    const float* scale_factors; int nlevels;
};

// what both forms check, in this order: the counts, then (an empty call returns PSLFE_OK before this) the arrays and nlevels
int upkeep_counts(const UpkeepHost& H, const char* who) {
    PSL_REQUIRE(H.M >= 0 && H.nkf >= 0, PSLFE_E_INVALID, "%s: M = %d, nkf = %d", who, H.M, H.nkf);
    return PSLFE_OK;
}
int upkeep_arrays(const UpkeepHost& H, const char* who) {
    PSL_REQUIRE(H.nlevels >= 1 && H.nlevels <= PSLFE_MAX_LEVELS, PSLFE_E_INVALID, "%s: nlevels = %d (1..%d)", who, H.nlevels, PSLFE_MAX_LEVELS);
    PSL_REQUIRE(H.rows && H.obs_off && H.obs_kf && H.centres && H.ref_kf && H.ref_level && H.scale_factors, PSLFE_E_INVALID, "%s: NULL array",
                who);
    return PSLFE_OK;
}

// the host forms: offsets ascending from 0, every index inside its table
int upkeep_indices(const UpkeepHost& H, const char* who) {
    PSL_REQUIRE(H.obs_off[0] == 0, PSLFE_E_INVALID, "%s: obs_off[0] = %d, must be 0", who, H.obs_off[0]);
    for (int i = 0; i < H.M; ++i) PSL_REQUIRE(H.obs_off[i + 1] >= H.obs_off[i], PSLFE_E_INVALID, "%s: obs_off descends at %d", who, i);
    const int nobs = H.obs_off[H.M];
    for (int o = 0; o < nobs; ++o)
        PSL_REQUIRE(H.obs_kf[o] >= 0 && H.obs_kf[o] < H.nkf, PSLFE_E_INVALID, "%s: obs_kf[%d] = %d outside [0, %d)", who, o, H.obs_kf[o], H.nkf);
    for (int i = 0; i < H.M; ++i) {
        if (H.obs_off[i + 1] == H.obs_off[i] || (H.skip && H.skip[i])) continue;   // a row that is not refreshed: its reference is not read
        PSL_REQUIRE(H.ref_kf[i] >= 0 && H.ref_kf[i] < H.nkf, PSLFE_E_INVALID, "%s: ref_kf[%d] = %d outside [0, %d)", who, i, H.ref_kf[i], H.nkf);
        PSL_REQUIRE(H.ref_level[i] >= 0 && H.ref_level[i] < H.nlevels, PSLFE_E_INVALID, "%s: ref_level[%d] = %d outside [0, %d)", who, i,
                    H.ref_level[i], H.nlevels);
    }
    return PSLFE_OK;
}

template <class U>
int upkeep_launch(pslfe_kf* k, const UpkeepHost& D, const float* scale_factors, const char* stage) {
    UpkeepArgs A;
    A.rows = D.rows; A.M = D.M; A.obs_off = D.obs_off; A.obs_kf = D.obs_kf; A.centres = D.centres; A.ref_kf = D.ref_kf;
    A.ref_level = D.ref_level; A.skip = D.skip; A.nlevels = D.nlevels;
    for (int l = 0; l < PSLFE_MAX_LEVELS; ++l) A.scale[l] = l < D.nlevels ? scale_factors[l] : 0.f;
    pslfe_ctx* ctx = k->ctx;
    const int blocks = (D.M + PSL_UPK_BS - 1) / PSL_UPK_BS;
    {
        PSL_STAGE_BEGIN(ctx, stage);
        if (k->upkeep_sum == PSLFE_UPKEEP_SUM_TILED) k_upkeep_tiled<U><<<blocks, PSL_UPK_BS, 0, ctx->stream>>>(A);
        else k_upkeep_walk<U><<<blocks, PSL_UPK_BS, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, stage);
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

template <class U, class Row>
int upkeep_device(pslfe_kf* k, const UpkeepHost& H, const char* who, const char* stage) {
    if (int rc = upkeep_counts(H, who)) return rc;
    if (H.M == 0) return PSLFE_OK;
    if (int rc = upkeep_arrays(H, who)) return rc;
    PSL_REQUIRE(k, PSLFE_E_INVALID, "%s: NULL handle", who);
    PSL_HIP(hipSetDevice(k->ctx->device));
    return upkeep_launch<U>(k, H, H.scale_factors, stage);
}

template <class U, class Row>
int upkeep_host(pslfe_kf* k, const UpkeepHost& H, const char* who, const char* stage) {
    if (int rc = upkeep_counts(H, who)) return rc;
    if (H.M == 0) return PSLFE_OK;
    UpkeepHost C = H;   // without observations or keyframes there is nothing to read behind these two
    static const int32_t none_i = 0;
    static const float none_f = 0.f;
    if (H.obs_off && H.obs_off[H.M] == 0 && !C.obs_kf) C.obs_kf = &none_i;
    if (H.nkf == 0 && !C.centres) C.centres = &none_f;
    if (int rc = upkeep_arrays(C, who)) return rc;
    if (int rc = upkeep_indices(H, who)) return rc;
    PSL_REQUIRE(k, PSLFE_E_INVALID, "%s: NULL handle", who);
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    const size_t nobs = (size_t)H.obs_off[H.M];
    hipError_t e = hipSuccess;
    UpkeepHost D = H;
    Row* d_rows = psl_scratch_up(ctx, static_cast<const Row*>(H.rows), (size_t)H.M, st, &e);
    D.rows = d_rows;
    D.obs_off = psl_scratch_up(ctx, H.obs_off, (size_t)H.M + 1, st, &e);
    D.obs_kf = psl_scratch_up(ctx, nobs ? H.obs_kf : nullptr, nobs, st, &e);
    D.centres = psl_scratch_up(ctx, H.nkf ? H.centres : nullptr, (size_t)H.nkf * 3, st, &e);
    D.ref_kf = psl_scratch_up(ctx, H.ref_kf, (size_t)H.M, st, &e);
    D.ref_level = psl_scratch_up(ctx, H.ref_level, (size_t)H.M, st, &e);
    D.skip = H.skip ? psl_scratch_up(ctx, H.skip, (size_t)H.M, st, &e) : nullptr;
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    if (int rc = upkeep_launch<U>(k, D, H.scale_factors, stage)) return rc;
    PSL_HIP(hipMemcpyAsync(H.rows, d_rows, (size_t)H.M * sizeof(Row), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_kf_set_upkeep_sum(pslfe_kf* k, int layout) {
    PSL_REQUIRE(k, PSLFE_E_INVALID, "pslfe_kf_set_upkeep_sum: NULL handle");
    PSL_REQUIRE(layout == PSLFE_UPKEEP_SUM_WALK || layout == PSLFE_UPKEEP_SUM_TILED, PSLFE_E_INVALID, "pslfe_kf_set_upkeep_sum: layout = %d", layout);
    k->upkeep_sum = layout;
    return PSLFE_OK;
}

int pslfe_kf_update_normal_and_depth(pslfe_kf* k, PslMapPointGeom* mp, int M, const int32_t* obs_off, const int32_t* obs_kf, const float* centres,
                                     int nkf, const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* skip, const float* scale_factors,
                                     int nlevels) {
    const UpkeepHost H = {mp, M, obs_off, obs_kf, centres, nkf, ref_kf, ref_level, skip, scale_factors, nlevels};
    return upkeep_host<UpkPoint, PslMapPointGeom>(k, H, "pslfe_kf_update_normal_and_depth", "kf.update_normal_and_depth");
}

int pslfe_kf_update_normal_and_depth_device(pslfe_kf* k, PslMapPointGeom* d_mp, int M, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                            const float* d_centres, int nkf, const int32_t* d_ref_kf, const int32_t* d_ref_level,
                                            const uint8_t* d_skip, const float* scale_factors, int nlevels) {
    const UpkeepHost H = {d_mp, M, d_obs_off, d_obs_kf, d_centres, nkf, d_ref_kf, d_ref_level, d_skip, scale_factors, nlevels};
    return upkeep_device<UpkPoint, PslMapPointGeom>(k, H, "pslfe_kf_update_normal_and_depth_device", "kf.update_normal_and_depth");
}

int pslfe_kf_line_update_average_dir(pslfe_kf* k, PslMapLineGeom* ml, int M, const int32_t* obs_off, const int32_t* obs_kf, const float* centres,
                                     int nkf, const int32_t* ref_kf, const int32_t* ref_level, const uint8_t* skip, const float* scale_factors,
                                     int nlevels) {
    const UpkeepHost H = {ml, M, obs_off, obs_kf, centres, nkf, ref_kf, ref_level, skip, scale_factors, nlevels};
    return upkeep_host<UpkLine, PslMapLineGeom>(k, H, "pslfe_kf_line_update_average_dir", "kf.line_update_average_dir");
}

int pslfe_kf_line_update_average_dir_device(pslfe_kf* k, PslMapLineGeom* d_ml, int M, const int32_t* d_obs_off, const int32_t* d_obs_kf,
                                            const float* d_centres, int nkf, const int32_t* d_ref_kf, const int32_t* d_ref_level,
                                            const uint8_t* d_skip, const float* scale_factors, int nlevels) {
    const UpkeepHost H = {d_ml, M, d_obs_off, d_obs_kf, d_centres, nkf, d_ref_kf, d_ref_level, d_skip, scale_factors, nlevels};
    return upkeep_device<UpkLine, PslMapLineGeom>(k, H, "pslfe_kf_line_update_average_dir_device", "kf.line_update_average_dir");
}

int pslfe_kf_scene_median_depth(pslfe_kf* k, const PslPose* Tcw, int K, const float* x, const int32_t* off, int q, float* depth) {
    static const char* who = "pslfe_kf_scene_median_depth";
    PSL_REQUIRE(K >= 0, PSLFE_E_INVALID, "%s: K = %d", who, K);
    if (K == 0) return PSLFE_OK;
    PSL_REQUIRE(Tcw && off && depth, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(q >= 1, PSLFE_E_INVALID, "%s: q = %d", who, q);
    PSL_REQUIRE(off[0] == 0, PSLFE_E_INVALID, "%s: off[0] = %d, must be 0", who, off[0]);
    for (int i = 0; i < K; ++i) PSL_REQUIRE(off[i + 1] >= off[i], PSLFE_E_INVALID, "%s: off descends at %d", who, i);
    const size_t n = (size_t)off[K];
    PSL_REQUIRE(n == 0 || x, PSLFE_E_INVALID, "%s: NULL positions", who);
    PSL_REQUIRE(k, PSLFE_E_INVALID, "%s: NULL handle", who);
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const PslPose* d_T = psl_scratch_up(ctx, Tcw, (size_t)K, st, &e);
    const float* d_x = psl_scratch_up(ctx, n ? x : nullptr, n * 3, st, &e);
    const int32_t* d_off = psl_scratch_up(ctx, off, (size_t)K + 1, st, &e);
    float* d_depth = psl_scratch_up(ctx, (const float*)nullptr, (size_t)K, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    {
        PSL_STAGE_BEGIN(ctx, "kf.scene_median_depth");
        k_scene_median_depth<<<K, 256, 0, st>>>(d_T, d_x, d_off, q, d_depth);
        PSL_STAGE_END(ctx, "kf.scene_median_depth");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(depth, d_depth, (size_t)K * sizeof(float), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

}  // extern "C"
