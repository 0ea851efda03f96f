// libpslfe: the line half of LocalMapping at keyframe rate, for a set of keyframes in one call.  Product code.
// Reference behaviour reproduced:
//   LSDmatcher::Fuse(pKF, vpMapLines, th), projection and search    add_src/LSDmatcher.cpp:865-958   (K keyframes x M map lines)
//   KeyFrame::IsInImage                                              src/KeyFrame.cc:726-729
//   MapLine::PredictScale                                            add_src/MapLine.cpp:381-390
//   KeyFrame::GetLinesInArea                                         src/KeyFrame.cc:857-891
//   LSDmatcher::SearchForTriangulation, both live overloads          add_src/LSDmatcher.cpp:705-781   (one keyframe x K neighbours)
//   LSDmatcher::FrameBFMatch + lineDescriptorMAD                     add_src/LSDmatcher.cpp:492-516, 660-685
// Conventions: include/pslfe.h above pslfe_kf_line_project; helpers: proj_kernels.h, kf_line_kernels.h; differences from the frame
// line forms: DESIGN.md §5.0h.
//
// Projection: one thread per (keyframe, map line), keyframes on blockIdx.y, rows not compacted (the host tail indexes by map line).
// A thread reads 80 B of geometry as five 16-byte loads and one skip byte and writes 24 B.  The reference leaves Fuse at the first
// line behind the camera (`return false`, :890-891): stop[k] is the smallest such line, found by atomicMin in the workgroup and
// then in memory, and k_kf_line_mask drops the rows at and after it once it is known.
// Search: one workgroup per (keyframe, chunk of map lines), one wave per map line; the keyframe's keylines are staged in LDS once
// per workgroup when they fit.
// Triangulation: the 2K FrameBFMatch directions run side by side on blockIdx.y of the kNN kernel and as the workgroups of the gate
// kernel; a third kernel applies the mutual test and the GetMapLine filter.
#include <limits.h>
#include <string.h>

#include "pslfe_internal.h"
#include "psl_device_math.h"

#include "match_kernels.h"
#include "proj_kernels.h"
#include "kf_project.h"
#include "kf_line_kernels.h"
#include "triangulate_kernels.h"

#define PSL_KLP_BS 256
#define PSL_KLF_LDS_MAX 512   // keylines of one keyframe staged in LDS (52 B each: 26 KB); more are read from global memory
#define PSL_KLF_CHUNK 16      // map lines per workgroup of the search: 4 per wave

static_assert(sizeof(PslPose) == 48 && sizeof(PslMapLineGeom) == 80 && sizeof(PslLineFuseQuery) == 24, "keyframe line projection PODs");

struct KfLineProjArgs {
    const PslPose* Tcw;
    float* ow;            // [K][3]
    const double2* ml;    // PslMapLineGeom rows as five 16-byte parts
    const uint8_t* skip;  // [K][M] or NULL
    int M;
    uint2* q;             // PslLineFuseQuery rows as three 8-byte parts
    int32_t* level;       // [K][M] or NULL
    int32_t* stop;        // [K]
};

__device__ __forceinline__ void psl_line_fuse_row_store(uint2* q, size_t row, float u1, float v1, float u2, float v2, float radius, int level) {
    q[3 * row] = make_uint2(__float_as_uint(u1), __float_as_uint(v1));
    q[3 * row + 1] = make_uint2(__float_as_uint(u2), __float_as_uint(v2));
    q[3 * row + 2] = make_uint2(__float_as_uint(radius), (uint32_t)level);
}

__global__ __launch_bounds__(PSL_KLP_BS) void k_kf_line_project(KfLineProjArgs A, ProjParams P) {
    __shared__ float s_pose[12 + 3 + PSLFE_MAX_LEVELS];
    __shared__ int s_stop;
    const int k = blockIdx.y, tid = threadIdx.x;
    if (tid < 12) s_pose[tid] = reinterpret_cast<const float*>(A.Tcw + k)[tid];
    else if (tid < 15) s_pose[tid] = A.ow[3 * k + tid - 12];
    else if (tid < 15 + PSLFE_MAX_LEVELS) s_pose[tid] = P.scale[tid - 15];
    if (tid == 0) s_stop = INT_MAX;
    __syncthreads();
    const int i = blockIdx.x * PSL_KLP_BS + tid;
    const size_t row = (size_t)k * A.M + (size_t)i;
    const float* R = s_pose;
    const float* t = s_pose + 9;
    const float* Ow = s_pose + 12;
    const float* scale = s_pose + 15;
    const PslCamera& C = P.cam;

    int lvl = INT_MIN;
    float u1 = 0.f, v1 = 0.f, u2 = 0.f, v2 = 0.f, radius = -1.0f;
    int qlevel = 0;
    bool behind = false;
    if (i < A.M && !(A.skip && A.skip[row])) {   // NULL, isBad(), IsInKeyFrame(pKF) (:869-873)
        const double2* G = A.ml + 5 * (size_t)i;
        const double2 g0 = G[0], g1 = G[1], g2 = G[2], g3 = G[3], g4 = G[4];  // sp0 sp1 | sp2 ep0 | ep1 ep2 | n0 n1 | n2 (min_dist max_dist)
        const float SP[3] = {(float)g0.x, (float)g0.y, (float)g1.x};            // Mat_<float> initialisers (:877-878)
        const float EP[3] = {(float)g1.y, (float)g2.x, (float)g2.y};
        const float min_dist = __int_as_float(__double2loint(g4.y)), max_dist = __int_as_float(__double2hiint(g4.y));
        const float SPcX = psl_affine_row(R[0], R[1], R[2], SP[0], SP[1], SP[2], t[0]);
        const float SPcY = psl_affine_row(R[3], R[4], R[5], SP[0], SP[1], SP[2], t[1]);
        const float SPcZ = psl_affine_row(R[6], R[7], R[8], SP[0], SP[1], SP[2], t[2]);
        const float EPcX = psl_affine_row(R[0], R[1], R[2], EP[0], EP[1], EP[2], t[0]);
        const float EPcY = psl_affine_row(R[3], R[4], R[5], EP[0], EP[1], EP[2], t[1]);
        const float EPcZ = psl_affine_row(R[6], R[7], R[8], EP[0], EP[1], EP[2], t[2]);
        behind = SPcZ < 0.0f || EPcZ < 0.0f;   // `return false` (:890-891); a depth of 0, -0 or NaN goes on and fails IsInImage
        if (!behind) {
            const float invz1 = PSL_FDIV(1.0f, SPcZ);
            const float pu1 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fx, SPcX), invz1), C.cx);
            const float pv1 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fy, SPcY), invz1), C.cy);
            const float invz2 = PSL_FDIV(1.0f, EPcZ);
            const float pu2 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fx, EPcX), invz2), C.cx);
            const float pv2 = PSL_FADD(PSL_FMUL(PSL_FMUL(C.fy, EPcY), invz2), C.cy);
            bool ok = pu1 >= P.minX && pu1 < P.maxX && pv1 >= P.minY && pv1 < P.maxY;   // KeyFrame::IsInImage
            ok = ok && pu2 >= P.minX && pu2 < P.maxX && pv2 >= P.minY && pv2 < P.maxY;
            if (ok) {
                float OM[3];   // 0.5*(SP+EP) - Ow (:911): a float sum, an exact halving, a float difference
#pragma unroll
                for (int c = 0; c < 3; ++c) OM[c] = PSL_FSUB(PSL_FMUL(0.5f, PSL_FADD(SP[c], EP[c])), Ow[c]);
                const float dist = psl_norm3(OM[0], OM[1], OM[2]);
                const float maxD = PSL_FMUL(1.2f, max_dist), minD = PSL_FMUL(0.8f, min_dist);
                ok = !(dist < minD || dist > maxD);                                       // :914
                // `OM.dot(pn) < 0.5 * dist` (:921): a double compare
                ok = ok && !(psl_dot3(OM[0], OM[1], OM[2], (float)g3.x, (float)g3.y, (float)g4.x) < PSL_DMUL(0.5, (double)dist));
                if (ok) {
                    lvl = psl_line_level(PSL_FDIV(max_dist, dist), P.log_scale_factor);
                    if (lvl >= 0 && lvl < P.nlevels) {   // outside: the reference reads mvScaleFactorsLine out of range; dropped here
                        u1 = pu1; v1 = pv1; u2 = pu2; v2 = pv2;
                        radius = PSL_FMUL(P.th, scale[lvl]);
                        qlevel = lvl;
                    }
                }
            }
        }
    }
    const uint64_t b = __ballot(behind);
    if (b && (tid & 63) == 0) atomicMin(&s_stop, blockIdx.x * PSL_KLP_BS + (tid & ~63) + __ffsll((unsigned long long)b) - 1);
    __syncthreads();
    if (tid == 0 && s_stop != INT_MAX) atomicMin(A.stop + k, s_stop);
    if (i >= A.M) return;
    psl_line_fuse_row_store(A.q, row, u1, v1, u2, v2, radius, qlevel);
    if (A.level) A.level[row] = lvl;
}

// rows i >= stop[k] are the ones the reference never reached
__global__ __launch_bounds__(PSL_KLP_BS) void k_kf_line_mask(KfLineProjArgs A) {
    const int k = blockIdx.y, i = blockIdx.x * PSL_KLP_BS + threadIdx.x;
    if (i >= A.M || i < A.stop[k]) return;
    const size_t row = (size_t)k * A.M + (size_t)i;
    psl_line_fuse_row_store(A.q, row, 0.f, 0.f, 0.f, 0.f, -1.0f, 0);
    if (A.level) A.level[row] = INT_MIN;
}

struct LineFuseSetArgs {
    const PslKeyLine* kls;
    const int32_t* kl_off;    // [K + 1]
    const uint8_t* desc;
    const int32_t* desc_off;  // [K + 1]
    const PslLineFuseQuery* q;  // [K][M]
    const uint8_t* qdesc;       // [M][32]
    int M;
    int* best_idx;
    int* best_dist;
};

// K keyframes x M map lines: the twin of k_line_fuse_best.  Workgroup (x, k) searches map lines x*CHUNK .. of keyframe k, a wave
// takes every fourth of them; the keyframe's keylines, reduced to what the loop reads, and its descriptor rows are staged once.
__global__ __launch_bounds__(256) void k_line_fuse_best_set(LineFuseSetArgs A) {
    __shared__ float4 s_geo[PSL_KLF_LDS_MAX];
    __shared__ int s_oct[PSL_KLF_LDS_MAX];
    __shared__ uint4 s_desc[PSL_KLF_LDS_MAX * 2];
    const int k = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int o0 = A.kl_off[k], n = A.kl_off[k + 1] - o0;
    const int d0 = A.desc_off[k], ndesc = A.desc_off[k + 1] - d0;
    const PslKeyLine* kls = A.kls + o0;
    const uint8_t* desc = A.desc + (size_t)d0 * 32;
    const bool staged = n <= PSL_KLF_LDS_MAX;   // uniform over the workgroup
    if (staged) {
        for (int j = tid; j < n; j += 256) {
            const PslKeyLine kl = kls[j];
            const float2 d = psl_keyline_dir(kl);
            s_geo[j] = make_float4(kl.pt_x, kl.pt_y, d.x, d.y);
            s_oct[j] = kl.octave;
        }
        const int nd = min(n, ndesc) * 2;
        const uint4* D = reinterpret_cast<const uint4*>(desc);
        for (int j = tid; j < nd; j += 256) s_desc[j] = D[j];
        __syncthreads();
    }
    const int i0 = blockIdx.x * PSL_KLF_CHUNK;
    for (int w = wave; w < PSL_KLF_CHUNK; w += 4) {
        const int i = i0 + w;
        if (i >= A.M) break;
        const size_t row = (size_t)k * A.M + (size_t)i;
        const PslLineFuseQuery q = A.q[row];
        const uint8_t* qd = A.qdesc + (size_t)i * 32;
        if (staged) {
            const LineFuseLds S = {s_geo, s_oct, s_desc};
            psl_line_fuse_row(S, n, ndesc, q, qd, lane, A.best_idx + row, A.best_dist + row);
        } else {
            const LineFuseGlobal S = {kls, reinterpret_cast<const uint32_t*>(desc)};
            psl_line_fuse_row(S, n, ndesc, q, qd, lane, A.best_idx + row, A.best_dist + row);
        }
    }
}

// ---- SearchForTriangulation against K neighbours ---------------------------------------------------------------------------
struct LineTriArgs {
    const uint8_t* desc1; int n1;
    const uint8_t* desc2; const int32_t* off2; int K;
    const uint8_t* has1; const uint8_t* has2;  // may be NULL
    int* knn_idx; int* knn_dist; float* mad;   // [2 * (K*n1 + off2[K])]: forward rows of neighbour k at k*n1, reverse rows at K*n1 + off2[k]
    int* lm;                                   // FrameBFMatch results, same rows
    float nnratio, TH;
    int mutual;
    int* match; int* nmatches;
};

// FrameBFMatch direction d: 2k = KF1's lines against neighbour k, 2k + 1 = the reverse
struct LineTriDir {
    const uint8_t* q; const uint8_t* t;
    int nq, nt;
    size_t row0;
};
__device__ __forceinline__ LineTriDir psl_line_tri_dir(const LineTriArgs& A, int d) {
    const int k = d >> 1, o = A.off2[k], n2 = A.off2[k + 1] - o;
    LineTriDir D;
    if (d & 1) { D.q = A.desc2 + (size_t)o * 32; D.nq = n2; D.t = A.desc1; D.nt = A.n1; D.row0 = (size_t)A.K * A.n1 + (size_t)o; }
    else { D.q = A.desc1; D.nq = A.n1; D.t = A.desc2 + (size_t)o * 32; D.nt = n2; D.row0 = (size_t)k * A.n1; }
    return D;
}

// knnMatch(k = 2) of every direction: the twin of k_hamming_knn2, one wave per query row, directions on blockIdx.y
__global__ __launch_bounds__(256) void k_line_tri_knn2(LineTriArgs A, int dstep) {
    const LineTriDir D = psl_line_tri_dir(A, blockIdx.y * dstep);
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (qi >= D.nq || D.nt < 2) return;   // knnMatch(k = 2) needs two train rows: no match (pslfe_line_frame_bf_match)
    psl_knn2_row(D.q + (size_t)qi * 32, D.t, D.nt, lane, A.knn_idx + 2 * (D.row0 + qi), A.knn_dist + 2 * (D.row0 + qi));
}

// MAD and gates of every direction: the twin of k_frame_bf_gate, one workgroup per direction
__global__ __launch_bounds__(256) void k_line_tri_gate(LineTriArgs A, int dstep) {
    __shared__ float s_med;
    const LineTriDir D = psl_line_tri_dir(A, blockIdx.x * dstep);
    if (D.nt < 2) {
        for (int i = threadIdx.x; i < D.nq; i += 256) A.lm[D.row0 + i] = -1;
        return;
    }
    if (D.nq <= 0) return;
    psl_frame_bf_gate(A.knn_idx + 2 * D.row0, A.knn_dist + 2 * D.row0, D.nq, A.nnratio, A.TH, A.mad + 2 * D.row0, A.lm + D.row0, &s_med);
}

// the loop of SearchForTriangulation (:725-740 / :764-778); nmatches is zero on entry
__global__ __launch_bounds__(256) void k_line_tri_pairs(LineTriArgs A) {
    const int k = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const int o = A.off2[k], n2 = A.off2[k + 1] - o;
    bool good = false;
    if (i < A.n1) {
        const int j = A.lm[(size_t)k * A.n1 + i];
        good = j >= 0 && j < n2;
        if (good && A.mutual) good = A.lm[(size_t)A.K * A.n1 + (size_t)o + j] == i;
        if (good && ((A.has1 && A.has1[i]) || (A.has2 && A.has2[o + j]))) good = false;   // GetMapLine(i) || GetMapLine(j)
        A.match[(size_t)k * A.n1 + i] = good ? j : -1;
    }
    const int c = __popcll(__ballot(good));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(A.nmatches + k, c);
}

// ---- CreateNewMapLines2 (src/LocalMapping.cc:554-757) behind the search -------------------------------------------------------------------
// one thread per line of KF1 walks the neighbours in order: the only dependence is "this line has its map line by now"
__global__ __launch_bounds__(256) void k_new_lines_walk(PslTriLineSet S) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < S.n1) psl_tri_line_walk(&S, i);
}
struct NewLinesList {
    PslTriLineSet S;
    int kf1;
    int* nmatches;
    PslNewMapLine* newl;
    int* nnew;
    PslMapLineGeom* geom;   // may be nullptr
    int* obs_off;           // the four observation arrays: all or none
    int* obs_kf;
    int* ref_kf;
    int* ref_level;
};
// the list in creation order (k ascending, idx1 ascending) and the counts; one workgroup
__global__ __launch_bounds__(256) void k_new_lines_list(NewLinesList L) {
    __shared__ int s_w[4];
    const PslTriLineSet& S = L.S;
    const int tid = threadIdx.x, n1 = S.n1;
    const int per = (n1 + 255) / 256, i0 = tid * per, i9 = min(i0 + per, n1);
    int nnew = 0;
    for (int k = 0; k < S.K; ++k) {
        int nm = 0, cnt = 0, total;
        for (int i = i0; i < i9; ++i) { nm += S.match[(size_t)k * n1 + i] >= 0; cnt += S.created_by[i] == k; }
        psl_block_scan_256(nm, s_w, &total);
        if (tid == 0) L.nmatches[k] = total;
        int pos = nnew + psl_block_scan_256(cnt, s_w, &total);
        for (int i = i0; i < i9; ++i) {
            if (S.created_by[i] != k) continue;
            const size_t row = (size_t)k * n1 + i;
            PslNewMapLine nl;
            PslMapLineGeom g;
            g.normal[0] = g.normal[1] = g.normal[2] = 0.0; g.min_dist = g.max_dist = 0.f;
#pragma unroll
            for (int c = 0; c < 3; ++c) { nl.sp[c] = S.sp[3 * row + c]; nl.ep[c] = S.ep[3 * row + c]; g.sp[c] = (double)nl.sp[c]; g.ep[c] = (double)nl.ep[c]; }
            nl.k = k; nl.idx1 = i; nl.idx2 = S.match[row];
            L.newl[pos] = nl;
            if (L.geom) L.geom[pos] = g;
            if (L.obs_kf) {
                const PslTriNeighbour* nb = S.nb + k;
                L.obs_kf[2 * pos] = nb->kf_first ? nb->kf : L.kf1;
                L.obs_kf[2 * pos + 1] = nb->kf_first ? L.kf1 : nb->kf;
                L.ref_kf[pos] = L.kf1;
                L.ref_level[pos] = S.kls1[i].octave;
            }
            ++pos;
        }
        nnew += total;
    }
    if (tid == 0) *L.nnew = nnew;
    if (L.obs_off)
        for (int r = tid; r <= n1; r += 256) L.obs_off[r] = 2 * min(r, nnew);
}

// ---------------------------------------------------------------------------------------------
namespace {

// The argument checks of both Fuse entry points.  The counts come first: an empty call (K == 0 or M == 0) is PSLFE_OK whatever else it
// passes, and the caller returns on it before the other checks.
int line_counts(int K, int M, const char* who) {
    PSL_REQUIRE(K >= 0 && M >= 0 && (double)K * (double)M <= (double)INT_MAX && K <= 65535, PSLFE_E_INVALID, "%s: K = %d, M = %d", who, K, M);
    return PSLFE_OK;
}

// K + 1 ascending, non-negative entries
int check_offsets(const int32_t* off, int K, const char* what, const char* who) {
    PSL_REQUIRE(off, PSLFE_E_INVALID, "%s: NULL %s", who, what);
    PSL_REQUIRE(off[0] >= 0, PSLFE_E_INVALID, "%s: %s[0] = %d", who, what, off[0]);
    for (int k = 0; k < K; ++k) PSL_REQUIRE(off[k + 1] >= off[k], PSLFE_E_INVALID, "%s: %s descends at %d", who, what, k);
    return PSLFE_OK;
}

// after psl_scratch_begin: uploads poses, map lines and skip, takes the outputs from the arena and launches centres, projection, mask
int line_project_upload(pslfe_ctx* ctx, const ProjParams& P, const PslPose* Tcw, int K, const PslMapLineGeom* ml, const uint8_t* skip, int M,
                        bool want_level, KfLineProjArgs* A, const char* who) {
    hipStream_t st = ctx->stream;
    const size_t rows = (size_t)K * M;
    hipError_t e = hipSuccess;
    A->Tcw = psl_scratch_up(ctx, Tcw, K, st, &e);
    A->ml = reinterpret_cast<const double2*>(psl_scratch_up(ctx, ml, M, st, &e));
    A->skip = skip ? psl_scratch_up(ctx, skip, rows, st, &e) : nullptr;
    A->M = M;
    A->ow = psl_scratch_up<float>(ctx, nullptr, (size_t)K * 3, st, &e);
    A->q = reinterpret_cast<uint2*>(psl_scratch_up<PslLineFuseQuery>(ctx, nullptr, rows, st, &e));
    A->level = want_level ? psl_scratch_up<int32_t>(ctx, nullptr, rows, st, &e) : nullptr;
    A->stop = psl_scratch_up<int32_t>(ctx, nullptr, K, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    const dim3 grid((M + PSL_KLP_BS - 1) / PSL_KLP_BS, K);
    {
        PSL_STAGE_BEGIN(ctx, "kf.line_project");
        psl_proj_centres_launch(st, A->Tcw, sizeof(PslPose), K, A->ow, A->stop, M);
        k_kf_line_project<<<grid, PSL_KLP_BS, 0, st>>>(*A, P);
        k_kf_line_mask<<<grid, PSL_KLP_BS, 0, st>>>(*A);
        PSL_STAGE_END(ctx, "kf.line_project");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_kf_line_project(pslfe_kf* k, const PslPose* Tcw, int K, const PslMapLineGeom* ml, const uint8_t* skip, int M, const PslCamera* cam,
                          float min_x, float min_y, float max_x, float max_y, const float* scale_factors_line, int nlevels,
                          float log_scale_factor_line, float th, PslLineFuseQuery* queries, int32_t* level, int32_t* stop) {
    static const char* who = "pslfe_kf_line_project";
    if (int rc = line_counts(K, M, who)) return rc;
    if (K == 0 || M == 0) return PSLFE_OK;
    ProjParams P;
    if (int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, scale_factors_line, nlevels, log_scale_factor_line, th, who))
        return rc;
    PSL_REQUIRE(Tcw && ml && queries && stop, PSLFE_E_INVALID, "%s: NULL poses, map lines or output", who);
    PSL_REQUIRE(k, PSLFE_E_INVALID, "%s: NULL handle", who);
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    const size_t rows = (size_t)K * M;
    KfLineProjArgs A;
    if (int rc = line_project_upload(ctx, P, Tcw, K, ml, skip, M, level != nullptr, &A, who)) return rc;
    PSL_HIP(hipMemcpyAsync(queries, A.q, rows * sizeof(PslLineFuseQuery), hipMemcpyDeviceToHost, st));
    if (level) PSL_HIP(hipMemcpyAsync(level, A.level, rows * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(stop, A.stop, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_line_fuse_keyframes(pslfe_kf* k, const PslPose* Tcw, int K, const PslKeyLine* kls, const int32_t* kl_off, const uint8_t* desc,
                                 const int32_t* desc_off, const PslMapLineGeom* ml, const uint8_t* mldesc, const uint8_t* skip, int M,
                                 const PslCamera* cam, float min_x, float min_y, float max_x, float max_y, const float* scale_factors_line,
                                 int nlevels, float log_scale_factor_line, float th, int32_t* best_idx, int32_t* best_dist,
                                 PslLineFuseQuery* queries, int32_t* stop) {
    static const char* who = "pslfe_kf_line_fuse_keyframes";
    if (int rc = line_counts(K, M, who)) return rc;
    if (K == 0 || M == 0) return PSLFE_OK;
    ProjParams P;
    if (int rc = psl_proj_params(&P, PSL_PROJ_NO_MODE, cam, min_x, min_y, max_x, max_y, scale_factors_line, nlevels, log_scale_factor_line, th, who))
        return rc;
    PSL_REQUIRE(Tcw && ml && mldesc && best_idx && best_dist && stop, PSLFE_E_INVALID, "%s: NULL argument", who);
    if (int rc = check_offsets(kl_off, K, "kl_off", who)) return rc;
    if (int rc = check_offsets(desc_off, K, "desc_off", who)) return rc;
    for (int i = 0; i < K; ++i)
        PSL_REQUIRE(kl_off[i + 1] - kl_off[i] <= 0xffff, PSLFE_E_INVALID, "%s: keyframe %d has %d keylines (max 65535)", who, i,
                    kl_off[i + 1] - kl_off[i]);
    PSL_REQUIRE((kl_off[K] == 0 || kls) && (desc_off[K] == 0 || desc), PSLFE_E_INVALID, "%s: NULL keylines or descriptors", who);
    PSL_REQUIRE(k, PSLFE_E_INVALID, "%s: NULL handle", who);
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    const size_t rows = (size_t)K * M;
    KfLineProjArgs A;
    if (int rc = line_project_upload(ctx, P, Tcw, K, ml, skip, M, false, &A, who)) return rc;
    hipError_t e = hipSuccess;
    LineFuseSetArgs S;
    const size_t nkl = (size_t)kl_off[K], nd = (size_t)desc_off[K];
    S.kls = psl_scratch_up(ctx, nkl ? kls : nullptr, nkl ? nkl : 1, st, &e);
    S.kl_off = psl_scratch_up(ctx, kl_off, (size_t)K + 1, st, &e);
    S.desc = psl_scratch_up(ctx, nd ? desc : nullptr, (nd ? nd : 1) * 32, st, &e);
    S.desc_off = psl_scratch_up(ctx, desc_off, (size_t)K + 1, st, &e);
    S.q = reinterpret_cast<const PslLineFuseQuery*>(A.q);
    S.qdesc = psl_scratch_up(ctx, mldesc, (size_t)M * 32, st, &e);
    S.M = M;
    S.best_idx = psl_scratch_up(ctx, (const int*)nullptr, rows, st, &e);
    S.best_dist = psl_scratch_up(ctx, (const int*)nullptr, rows, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    {
        PSL_STAGE_BEGIN(ctx, "kf.line_fuse_set");
        k_line_fuse_best_set<<<dim3((M + PSL_KLF_CHUNK - 1) / PSL_KLF_CHUNK, K), 256, 0, st>>>(S);
        PSL_STAGE_END(ctx, "kf.line_fuse_set");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(best_idx, S.best_idx, rows * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(best_dist, S.best_dist, rows * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(stop, A.stop, (size_t)K * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    if (queries) PSL_HIP(hipMemcpyAsync(queries, A.q, rows * sizeof(PslLineFuseQuery), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

namespace {
// the checks of the search, in its order; *done = 1: K == 0
int line_tri_check(const char* who, pslfe_kf* k, const uint8_t* desc1, int n1, const uint8_t* desc2, const int32_t* off2, int K, bool outputs, int* done) {
    *done = 0;
    PSL_REQUIRE(K >= 0 && K <= 32767 && n1 >= 0 && n1 < (1 << 20) && (double)K * (double)n1 <= (double)(INT_MAX / 4), PSLFE_E_INVALID,
                "%s: K = %d, n1 = %d", who, K, n1);
    if (K == 0) { *done = 1; return PSLFE_OK; }   // no neighbour: nothing to write
    PSL_REQUIRE(outputs && (n1 == 0 || desc1), PSLFE_E_INVALID, "%s: NULL argument", who);
    if (int rc = check_offsets(off2, K, "off2", who)) return rc;
    PSL_REQUIRE(off2[0] == 0, PSLFE_E_INVALID, "%s: off2[0] must be 0", who);
    for (int i = 0; i < K; ++i)
        PSL_REQUIRE(off2[i + 1] - off2[i] < (1 << 20), PSLFE_E_INVALID, "%s: neighbour %d has %d lines", who, i, off2[i + 1] - off2[i]);
    PSL_REQUIRE(off2[K] <= INT_MAX / 4, PSLFE_E_INVALID, "%s: %d neighbour lines", who, off2[K]);
    PSL_REQUIRE(off2[K] == 0 || desc2, PSLFE_E_INVALID, "%s: NULL neighbour descriptors", who);
    PSL_REQUIRE(k, PSLFE_E_INVALID, "%s: NULL handle", who);
    return PSLFE_OK;
}

// The launch chain of the search, n1 > 0, inside an open scratch scope: A->match [K*n1] and A->nmatches [K] stay on the device.  The
// descriptor and GetMapLine arrays are host arrays (uploaded) or, with on_device, device arrays.  With no neighbour line at all nothing
// is launched: rows of -1.
int line_tri_queue(const char* who, pslfe_ctx* ctx, const uint8_t* desc1, int n1, const uint8_t* has_mapline1, const uint8_t* desc2, const int32_t* off2,
                   const uint8_t* has_mapline2, int K, float nnratio, float TH, int mutual, bool on_device, LineTriArgs* out) {
    hipStream_t st = ctx->stream;
    const int n2all = off2[K];
    const size_t rows = (size_t)K * n1 + (size_t)n2all;
    hipError_t e = hipSuccess;
    LineTriArgs& A = *out;
    A.n1 = n1; A.K = K;
    A.off2 = psl_scratch_up(ctx, off2, (size_t)K + 1, st, &e);
    A.match = psl_scratch_up(ctx, (const int*)nullptr, (size_t)K * n1, st, &e);
    A.nmatches = psl_scratch_up(ctx, (const int*)nullptr, K, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    PSL_HIP(hipMemsetAsync(A.nmatches, 0, (size_t)K * sizeof(int), st));
    if (n2all == 0) {
        PSL_HIP(hipMemsetAsync(A.match, 0xff, (size_t)K * n1 * sizeof(int), st));
        return PSLFE_OK;
    }
    if (on_device) {
        A.desc1 = desc1; A.desc2 = desc2; A.has1 = has_mapline1; A.has2 = has_mapline2;
    } else {
        A.desc1 = psl_scratch_up(ctx, desc1, (size_t)n1 * 32, st, &e);
        A.desc2 = psl_scratch_up(ctx, desc2, (size_t)n2all * 32, st, &e);
        A.has1 = has_mapline1 ? psl_scratch_up(ctx, has_mapline1, n1, st, &e) : nullptr;
        A.has2 = has_mapline2 ? psl_scratch_up(ctx, has_mapline2, n2all, st, &e) : nullptr;
    }
    A.knn_idx = psl_scratch_up(ctx, (const int*)nullptr, rows * 2, st, &e);
    A.knn_dist = psl_scratch_up(ctx, (const int*)nullptr, rows * 2, st, &e);
    A.mad = psl_scratch_up(ctx, (const float*)nullptr, rows * 2, st, &e);
    A.lm = psl_scratch_up(ctx, (const int*)nullptr, rows, st, &e);
    A.nnratio = nnratio; A.TH = TH; A.mutual = mutual != 0;
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    int maxq = n1;
    if (A.mutual) for (int i = 0; i < K; ++i) maxq = off2[i + 1] - off2[i] > maxq ? off2[i + 1] - off2[i] : maxq;
    const int ndir = A.mutual ? 2 * K : K, dstep = A.mutual ? 1 : 2;   // without the mutual test the reverse directions are not read
    {
        PSL_STAGE_BEGIN(ctx, "kf.line_triangulation_set");
        k_line_tri_knn2<<<dim3((maxq + 3) / 4, ndir), 256, 0, st>>>(A, dstep);
        k_line_tri_gate<<<ndir, 256, 0, st>>>(A, dstep);
        k_line_tri_pairs<<<dim3((n1 + 255) / 256, K), 256, 0, st>>>(A);
        PSL_STAGE_END(ctx, "kf.line_triangulation_set");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

// D: the device arrays of the pair body and of the list; the search's inputs as line_tri_queue takes them
struct NewLinesDev {
    const PslKeyLine* kls1; const double* l3d1; const float* lineeq1; const PslKeyLine* kls2; const double* l3d2;
    int* match; int* status; float* sp; float* ep; int* nmatches; int* created_by; PslNewMapLine* newl; int* nnew; PslMapLineGeom* geom;
    int* obs_off; int* obs_kf; int* ref_kf; int* ref_level;
};
int new_lines_queue(const char* who, pslfe_ctx* ctx, const PslTriKeyFrame* kf1, int NL1, const uint8_t* desc1, const uint8_t* has1,
                    const PslTriNeighbour* nb, int K, const uint8_t* desc2, const int32_t* off2, const uint8_t* has2, float nnratio, float TH, int mutual,
                    const float* scale_factors, const float* level_sigma2, int nlevels, bool on_device, const NewLinesDev& D) {
    hipStream_t st = ctx->stream;
    LineTriArgs T;
    if (int rc = line_tri_queue(who, ctx, desc1, NL1, has1, desc2, off2, has2, K, nnratio, TH, mutual, on_device, &T)) return rc;
    std::vector<PslTriCam> cams((size_t)K + 1);   // the set-up is host arithmetic: the same IEEE operations as in the kernels
    for (int i = 0; i < K; ++i) psl_tri_cam_setup(&nb[i].Tcw, nb[i].fx, nb[i].fy, nb[i].cx, nb[i].cy, nb[i].mb, &cams[i]);
    psl_tri_cam_setup(&kf1->Tcw, kf1->fx, kf1->fy, kf1->cx, kf1->cy, kf1->mb, &cams[K]);
    hipError_t e = hipSuccess;
    NewLinesList L;
    PslTriLineSet& S = L.S;
    S.cams = psl_scratch_up(ctx, cams.data(), (size_t)K + 1, st, &e);
    S.nb = psl_scratch_up(ctx, nb, K, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    S.C1 = S.cams + K; S.K = K; S.n1 = NL1;
    S.kls1 = D.kls1; S.l3d1 = D.l3d1; S.lineeq1 = D.lineeq1; S.kls2 = D.kls2; S.l3d2 = D.l3d2; S.off2 = T.off2; S.match0 = T.match;
    for (int i = 0; i < PSL_TRI_LEVELS; ++i) { S.sf[i] = i < nlevels ? scale_factors[i] : 0.f; S.sig2[i] = i < nlevels ? level_sigma2[i] : 0.f; }
    S.ratioFactor = kf1->ratio_factor;
    S.match = D.match; S.status = D.status; S.sp = D.sp; S.ep = D.ep; S.created_by = D.created_by;
    L.kf1 = kf1->kf; L.nmatches = D.nmatches; L.newl = D.newl; L.nnew = D.nnew; L.geom = D.geom;
    L.obs_off = D.obs_off; L.obs_kf = D.obs_kf; L.ref_kf = D.ref_kf; L.ref_level = D.ref_level;
    {
        PSL_STAGE_BEGIN(ctx, "kf.new_lines");
        k_new_lines_walk<<<(NL1 + 255) / 256, 256, 0, st>>>(S);
        k_new_lines_list<<<1, 256, 0, st>>>(L);
        PSL_STAGE_END(ctx, "kf.new_lines");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}
// the checks behind the search's: *done = 1 when there is nothing to queue
int new_lines_check(const char* who, pslfe_kf* k, const PslTriKeyFrame* kf1, int NL1, const uint8_t* desc1, const PslTriNeighbour* nb, int K,
                    const uint8_t* desc2, const int32_t* off2, const float* scale_factors, const float* level_sigma2, int nlevels, bool outputs,
                    bool arrays, int* done) {
    if (int rc = line_tri_check(who, k, desc1, NL1, desc2, off2, K, outputs, done)) return rc;
    PSL_REQUIRE(NL1 <= 0xffff && K <= PSLFE_TRI_MAX_NEIGHBOURS, PSLFE_E_INVALID, "%s: NL1 = %d (max 65535), K = %d (max %d)", who, NL1, K,
                PSLFE_TRI_MAX_NEIGHBOURS);
    if (*done) return PSLFE_OK;
    PSL_REQUIRE(kf1 && nb && scale_factors && level_sigma2 && arrays, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(nlevels > 0 && nlevels <= PSL_TRI_LEVELS, PSLFE_E_INVALID, "%s: %d levels (max %d)", who, nlevels, PSL_TRI_LEVELS);
    return PSLFE_OK;
}
}  // namespace

int pslfe_kf_line_search_for_triangulation_keyframes(pslfe_kf* k, const uint8_t* desc1, int n1, const uint8_t* has_mapline1, const uint8_t* desc2,
                                                     const int32_t* off2, const uint8_t* has_mapline2, int K, float nnratio, float TH, int mutual,
                                                     int32_t* match, int32_t* nmatches) {
    static const char* who = "pslfe_kf_line_search_for_triangulation_keyframes";
    int done;
    if (int rc = line_tri_check(who, k, desc1, n1, desc2, off2, K, nmatches && (n1 == 0 || match), &done)) return rc;
    if (done) return PSLFE_OK;
    for (int i = 0; i < K; ++i) nmatches[i] = 0;
    if (n1 == 0) return PSLFE_OK;                        // ldesc1.rows == 0 (:715-716)
    for (size_t i = 0; i < (size_t)K * n1; ++i) match[i] = -1;
    if (off2[K] == 0) return PSLFE_OK;                   // every neighbour is empty
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    LineTriArgs A;
    if (int rc = line_tri_queue(who, ctx, desc1, n1, has_mapline1, desc2, off2, has_mapline2, K, nnratio, TH, mutual, false, &A)) return rc;
    PSL_HIP(hipMemcpyAsync(match, A.match, (size_t)K * n1 * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nmatches, A.nmatches, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_create_new_map_lines_device(pslfe_kf* k, const PslTriKeyFrame* kf1, int NL1, const uint8_t* d_desc1, const uint8_t* d_has_mapline1,
                                         const PslKeyLine* d_kls1, const double* d_lines3d1, const float* d_lineeq1, const PslTriNeighbour* nb, int K,
                                         const uint8_t* d_desc2, const int32_t* off2, const uint8_t* d_has_mapline2, const PslKeyLine* d_kls2,
                                         const double* d_lines3d2, float nnratio, float TH, int mutual, const float* scale_factors,
                                         const float* level_sigma2, int nlevels, int32_t* d_match, int32_t* d_status, float* d_sp, float* d_ep,
                                         int32_t* d_nmatches, int32_t* d_created_by, PslNewMapLine* d_newl, int32_t* d_nnew, PslMapLineGeom* d_geom,
                                         int32_t* d_obs_off, int32_t* d_obs_kf, int32_t* d_ref_kf, int32_t* d_ref_level) {
    static const char* who = "pslfe_kf_create_new_map_lines_device";
    int done;
    const bool arrays = d_nnew && d_obs_off && (NL1 == 0 || (d_kls1 && d_lines3d1 && d_lineeq1 && d_status && d_sp && d_ep && d_created_by && d_newl &&
                                                             d_geom && d_obs_kf && d_ref_kf && d_ref_level));
    if (int rc = new_lines_check(who, k, kf1, NL1, d_desc1, nb, K, d_desc2, off2, scale_factors, level_sigma2, nlevels, d_nmatches && (NL1 == 0 || d_match),
                                 arrays, &done))
        return rc;
    if (done) return PSLFE_OK;
    PSL_REQUIRE(off2[K] == 0 || (d_kls2 && d_lines3d2), PSLFE_E_INVALID, "%s: NULL neighbour lines", who);
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    if (int rc = psl_scratch_begin(ctx)) return rc;
    if (NL1 == 0) {
        PSL_HIP(hipMemsetAsync(d_nmatches, 0, (size_t)K * 4, ctx->stream));
        PSL_HIP(hipMemsetAsync(d_nnew, 0, 4, ctx->stream));
        PSL_HIP(hipMemsetAsync(d_obs_off, 0, 4, ctx->stream));
        return PSLFE_OK;
    }
    const NewLinesDev D = {d_kls1, d_lines3d1, d_lineeq1, d_kls2, d_lines3d2, d_match, d_status, d_sp, d_ep, d_nmatches, d_created_by, d_newl, d_nnew,
                           d_geom, d_obs_off, d_obs_kf, d_ref_kf, d_ref_level};
    return new_lines_queue(who, ctx, kf1, NL1, d_desc1, d_has_mapline1, nb, K, d_desc2, off2, d_has_mapline2, nnratio, TH, mutual, scale_factors,
                           level_sigma2, nlevels, true, D);
}

int pslfe_kf_create_new_map_lines(pslfe_kf* k, const PslTriKeyFrame* kf1, int NL1, const uint8_t* desc1, const uint8_t* has_mapline1,
                                  const PslKeyLine* kls1, const double* lines3d1, const float* lineeq1, const PslTriNeighbour* nb, int K,
                                  const uint8_t* desc2, const int32_t* off2, const uint8_t* has_mapline2, const PslKeyLine* kls2, const double* lines3d2,
                                  float nnratio, float TH, int mutual, const float* scale_factors, const float* level_sigma2, int nlevels,
                                  int32_t* match, int32_t* status, float* sp, float* ep, int32_t* nmatches, int32_t* created_by, PslNewMapLine* newl,
                                  int32_t* nnew, PslMapLineGeom* geom) {
    static const char* who = "pslfe_kf_create_new_map_lines";
    int done;
    const bool arrays = nnew && (NL1 == 0 || (kls1 && lines3d1 && lineeq1 && status && sp && ep && created_by && newl));
    if (int rc = new_lines_check(who, k, kf1, NL1, desc1, nb, K, desc2, off2, scale_factors, level_sigma2, nlevels, nmatches && (NL1 == 0 || match), arrays,
                                 &done))
        return rc;
    if (done) return PSLFE_OK;
    PSL_REQUIRE(off2[K] == 0 || (kls2 && lines3d2), PSLFE_E_INVALID, "%s: NULL neighbour lines", who);
    *nnew = 0;
    for (int i = 0; i < K; ++i) nmatches[i] = 0;
    if (NL1 == 0) return PSLFE_OK;
    pslfe_ctx* ctx = k->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const size_t n1 = NL1, rows = (size_t)K * n1, n2 = off2[K] ? off2[K] : 1;
    NewLinesDev D;
    D.kls1 = psl_scratch_up(ctx, kls1, n1, st, &e);
    D.l3d1 = psl_scratch_up(ctx, lines3d1, 6 * n1, st, &e);
    D.lineeq1 = psl_scratch_up(ctx, lineeq1, n1, st, &e);
    D.kls2 = psl_scratch_up(ctx, off2[K] ? kls2 : nullptr, n2, st, &e);
    D.l3d2 = psl_scratch_up(ctx, off2[K] ? lines3d2 : nullptr, 6 * n2, st, &e);
    D.match = psl_scratch_up(ctx, (const int*)nullptr, rows, st, &e);
    D.status = psl_scratch_up(ctx, (const int*)nullptr, rows, st, &e);
    D.sp = psl_scratch_up(ctx, (const float*)nullptr, rows * 3, st, &e);
    D.ep = psl_scratch_up(ctx, (const float*)nullptr, rows * 3, st, &e);
    D.nmatches = psl_scratch_up(ctx, (const int*)nullptr, K, st, &e);
    D.created_by = psl_scratch_up(ctx, (const int*)nullptr, n1, st, &e);
    D.newl = psl_scratch_up(ctx, (const PslNewMapLine*)nullptr, n1, st, &e);
    D.nnew = psl_scratch_up(ctx, (const int*)nullptr, 1, st, &e);
    D.geom = geom ? psl_scratch_up(ctx, (const PslMapLineGeom*)nullptr, n1, st, &e) : nullptr;
    D.obs_off = D.obs_kf = D.ref_kf = D.ref_level = nullptr;
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    PSL_HIP(hipMemsetAsync(D.newl, 0, n1 * sizeof(PslNewMapLine), st));   // the rows behind *nnew come back as zeros
    if (geom) PSL_HIP(hipMemsetAsync(D.geom, 0, n1 * sizeof(PslMapLineGeom), st));
    if (int rc = new_lines_queue(who, ctx, kf1, NL1, desc1, has_mapline1, nb, K, desc2, off2, has_mapline2, nnratio, TH, mutual, scale_factors,
                                 level_sigma2, nlevels, false, D))
        return rc;
    PSL_HIP(hipMemcpyAsync(match, D.match, rows * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(status, D.status, rows * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(sp, D.sp, rows * 12, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(ep, D.ep, rows * 12, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nmatches, D.nmatches, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(created_by, D.created_by, n1 * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(newl, D.newl, n1 * sizeof(PslNewMapLine), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nnew, D.nnew, 4, hipMemcpyDeviceToHost, st));
    if (geom) PSL_HIP(hipMemcpyAsync(geom, D.geom, n1 * sizeof(PslMapLineGeom), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

}  // extern "C"
