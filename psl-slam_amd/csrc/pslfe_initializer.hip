// libpslfe: Initializer (src/Initializer.cc), the two-view map initialisation of Tracking::MonocularInitialization
// (src/Tracking.cc:659-760), for K independent frame pairs in one launch.  Product code.
// Who owns what.  initializer_kernels.h holds everything a single thread computes - Normalize, the 8-point H and F, the scores of a row,
// the motion hypotheses, CheckRT for one row, the decision trees - and the reference's loop on one core (psl_init_initialize_host),
// which tools/dropin/init_main.cpp runs and tests/initializer_cases.py restates in numpy; glibc's rand(), the draw and this library's
// reading of OpenCV's Jacobi SVD are those of ransac_kernels.h, shared with the other RANSAC solvers.  Here: which thread computes which hypothesis and which row, the LDS copy of the matched rows, the error paths.
//
// Layout.  One workgroup of 256 threads per pair, resident through all stages.
//   rows        the matches are compacted in keypoint order by ballot (psl_wg_compact); the frame-1 keypoint of every row goes to an
//               arena array, and the first PSL_INIT_LDS_ROWS rows (u1 v1 u2 v2 i1: 5 words, an odd stride) to LDS.  A row beyond them is
//               read through that array from the keypoints where it is used.
//   Normalize   four lanes of wave 0, each its own two serial sums over all keypoints of its frame; meanwhile a lane of wave 1 seeds
//               the generator.
//   hypotheses  in blocks of PSL_INIT_B = 16 iterations: a lane of wave 1 draws the block's sets; then lane = hypothesis, the H of
//               iteration h on thread 8 h of waves 0-1 and the F of the same set on thread 128 + 8 h of waves 2-3, so the two models
//               never diverge inside a wave.  A 16x9 SVD needs 144 + 81 floats and 9 doubles, far more than a lane's registers, so the
//               workspaces lie in LDS, interleaved (element k of workspace s at word k * 32 + s): 32 workspaces are 28.8 KB + 2.3 KB.
//   scores      lane = hypothesis (lanes 0-15 of wave 0: H, of wave 2: F), walking the rows in order: every lane reads the same row,
//               an LDS broadcast, and each score is the reference's sequential float sum.  Thread 0 then takes the first strictly
//               greater score per model in iteration order.
//   flags       a row's flag under the winner is recomputed from the model wherever it is needed; nothing is stored.
//   motion      RH, the branch and the 4 or 8 (R, t) on thread 0, with the block's first workspace (stride 1).
//   CheckRT     per hypothesis, thread = row in chunks of 256; the 4x4 Jacobi of Triangulate runs per thread on 32 floats + 4 doubles
//               of the same LDS (32 KB + 8 KB, interleaved by thread).  nGood by ballot; the cosines go as ordered keys to an arena
//               array, and the element at sorted index min(50, n - 1) comes from a four-pass radix selection (exact: the value does
//               not depend on how it is found).  Only the accepted hypothesis is run once more to write vP3D and vbTriangulated.
// LDS: 32 KB + 8 KB workspaces, 10 KB rows, about 4 KB of block state: under the 64 KB a workgroup gets without an opt-in.
#include <string.h>

#include "pslfe_internal.h"
#include "match_kernels.h"
#include "proj_kernels.h"
#include "initializer_kernels.h"

#define PSL_INIT_BS 256
#define PSL_INIT_B 16
#define PSL_INIT_LDS_ROWS 512
#define PSL_INIT_WS_WORDS 8192   // max(2 * PSL_INIT_B * PSL_INIT_WS_F, PSL_INIT_BS * PSL_INIT_RT_F)
#define PSL_INIT_WD_WORDS 1024   // max(2 * PSL_INIT_B * PSL_INIT_WS_D, PSL_INIT_BS * PSL_INIT_RT_D)

static_assert(2 * PSL_INIT_B * PSL_INIT_WS_F <= PSL_INIT_WS_WORDS && PSL_INIT_BS * PSL_INIT_RT_F <= PSL_INIT_WS_WORDS, "float workspace");
static_assert(2 * PSL_INIT_B * PSL_INIT_WS_D <= PSL_INIT_WD_WORDS && PSL_INIT_BS * PSL_INIT_RT_D <= PSL_INIT_WD_WORDS, "double workspace");
static_assert(sizeof(PslKeyPoint) == 28, "a frame slot's keypoint record");

struct InitArgs {
    const float* keys1;            // pair p (or slot s) at keys + p * kpair floats
    const float* keys2;
    const int32_t* n1;             // array form: the counts; frames form: NULL
    const int32_t* n2;
    const int32_t* slot1;          // frames form: the slots of the pairs
    const int32_t* slot2;
    const FrameMeta* meta1;
    const FrameMeta* meta2;
    size_t ks, kpair1, kpair2;     // floats per keypoint, per pair / slot
    int kstride1, kstride2;
    const int32_t* matches;
    int mstride;
    PslCamera cam;
    float sigma;
    int max_its;
    uint32_t seed0;
    int32_t* row_i;                // arena [npairs][mstride]
    uint32_t* cos_keys;            // arena [npairs][mstride]
    PslInitResult* res;
    float* p3d;
    uint8_t* tri;
    int32_t* mout;
};

struct InitShared {
    PslInitNorm nm1, nm2;
    PslRsRand rand;
    int idx[PSL_INIT_B][8];
    float model[PSL_INIT_B][27];   // H21 H12 F21 of the block
    float score[2][PSL_INIT_B];
    float best[27];                // the winners
    float Rs[72], ts[24];
    PslInitRt rt;
    int hist[256];
    int part[4], cnt[4];
    int sel_k, nh, ok, best_h;
    uint32_t sel_prefix;
    PslInitResult o;               // thread 0's
};

// The key at sorted index min(50, n - 1) of keys[0..n), n >= 1, by a radix selection, most significant byte first.  Every thread calls
// it and gets the key; the keys were written before a barrier.
__device__ __forceinline__ uint32_t init_select_key(InitShared& sh, const uint32_t* keys, int n) {
    const int tid = threadIdx.x;
    if (tid == 0) { sh.sel_k = n - 1 < 50 ? n - 1 : 50; sh.sel_prefix = 0u; }
    for (int pass = 0; pass < 4; ++pass) {
        const int shift = 24 - 8 * pass;
        const uint32_t mask = pass == 0 ? 0u : (0xffffffffu << (shift + 8));
        sh.hist[tid] = 0;
        __syncthreads();
        const uint32_t prefix = sh.sel_prefix;
        for (int j = tid; j < n; j += PSL_INIT_BS) {
            const uint32_t k = keys[j];
            if ((k & mask) == prefix) atomicAdd(&sh.hist[(k >> shift) & 255u], 1);
        }
        __syncthreads();
        if (tid == 0) {
            int k = sh.sel_k, b = 0;
            while (b < 255 && k >= sh.hist[b]) { k -= sh.hist[b]; ++b; }
            sh.sel_k = k;
            sh.sel_prefix = prefix | ((uint32_t)b << shift);
        }
        __syncthreads();
    }
    return sh.sel_prefix;
}

// CheckRT of the hypothesis in sh.rt over the rows whose flag is set under model M; returns nGood, *parallax; with `write`, vP3D and
// vbTriangulated of the pair and *ntri.  Every thread calls it; every branch around a barrier is uniform.
__device__ __forceinline__ int init_check_rt(InitShared& sh, float* s_ws, double* s_wd, const PslInitRows& R, int N, int homography, float invS2,
                                             uint32_t* keys, bool write, float* p3d, uint8_t* tri, float* parallax, int* ntri) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int base = 0, tri_cnt = 0;
    for (int r0 = 0; r0 < N; r0 += PSL_INIT_BS) {   // uniform
        const int r = r0 + tid;
        int c = 0, i1 = 0;
        float p[3] = {0.f, 0.f, 0.f}, cosp = 0.f;
        if (r < N) {
            float q[4];
            i1 = psl_init_load(&R, r, q);
            if (psl_init_inlier(homography, sh.best + (homography ? 0 : 18), q, invS2))
                c = psl_init_rt_row<PSL_INIT_BS>(&sh.rt, q, s_ws + tid, s_wd + tid, p, &cosp);
        }
        int kept;
        const int pos = base + psl_wg_compact<PSL_INIT_BS>(c != 0, sh.cnt, &kept);
        base += kept;
        if (c) {
            keys[pos] = psl_init_cos_key(cosp);
            if (write) {
                p3d[3 * (size_t)i1] = p[0]; p3d[3 * (size_t)i1 + 1] = p[1]; p3d[3 * (size_t)i1 + 2] = p[2];
                if (c == 3) tri[i1] = 1;
            }
        }
        tri_cnt += __popcll(__ballot(c == 3));
    }
    if (lane == 0) sh.part[wave] = tri_cnt;
    __threadfence_block();
    __syncthreads();
    if (ntri) *ntri = sh.part[0] + sh.part[1] + sh.part[2] + sh.part[3];
    const int n = base;
    const float par = n > 0 ? psl_init_parallax(psl_init_cos_unkey(init_select_key(sh, keys, n))) : 0.f;   // uniform
    __syncthreads();
    *parallax = par;
    return n;
}

__global__ __launch_bounds__(PSL_INIT_BS) void k_init_solve(InitArgs A) {
    __shared__ float s_ws[PSL_INIT_WS_WORDS];
    __shared__ double s_wd[PSL_INIT_WD_WORDS];
    __shared__ float s_rows[PSL_INIT_LDS_ROWS * 5];
    __shared__ InitShared sh;
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    PslInitResult* res = A.res + p;
    int n1, n2;
    const float *k1, *k2;
    if (A.slot1) {
        const int s1 = A.slot1[p], s2 = A.slot2[p];
        n1 = A.meta1[s1].n; n2 = A.meta2[s2].n;
        k1 = A.keys1 + (size_t)s1 * A.kpair1; k2 = A.keys2 + (size_t)s2 * A.kpair2;
    } else {
        n1 = A.n1[p]; n2 = A.n2[p];
        k1 = A.keys1 + (size_t)p * A.kpair1; k2 = A.keys2 + (size_t)p * A.kpair2;
    }
    PslInitResult& o = sh.o;   // read and written by thread 0 alone
    if (tid == 0) memset(&o, 0, sizeof(o));
    if (n1 < 0 || n2 < 0 || n1 > A.kstride1 || n2 > A.kstride2 || n1 > A.mstride) {   // uniform; the record alone is written
        if (tid == 0) {
            o.status = (n1 < 0 || n2 < 0) ? PSLFE_E_INVALID : PSLFE_E_CAPACITY;
            *res = o;
        }
        return;
    }
    const int32_t* matches = A.matches + (size_t)p * A.mstride;
    int32_t* row_i = A.row_i + (size_t)p * A.mstride;
    uint32_t* keys = A.cos_keys + (size_t)p * A.mstride;
    float* p3d = A.p3d + 3 * (size_t)p * A.mstride;
    uint8_t* tri = A.tri + (size_t)p * A.mstride;
    int32_t* mout = A.mout ? A.mout + (size_t)p * A.mstride : nullptr;

    // mvMatches12 (:51-63): the rows in ascending keypoint order
    int N = 0, bad = 0;
    for (int i0 = 0; i0 < n1; i0 += PSL_INIT_BS) {   // uniform
        const int i = i0 + tid;
        int m = -1;
        if (i < n1) m = matches[i];
        if (m >= n2) { bad = 1; m = -1; }
        int kept;
        const int pos = N + psl_wg_compact<PSL_INIT_BS>(m >= 0, sh.cnt, &kept);
        N += kept;
        if (m >= 0) {
            row_i[pos] = i;
            if (pos < PSL_INIT_LDS_ROWS) {
                float* s = s_rows + 5 * pos;
                s[0] = k1[A.ks * (size_t)i]; s[1] = k1[A.ks * (size_t)i + 1];
                s[2] = k2[A.ks * (size_t)m]; s[3] = k2[A.ks * (size_t)m + 1];
                __builtin_memcpy(s + 4, &i, 4);
            }
        }
    }
    __threadfence_block();
    if (__syncthreads_or(bad)) {   // a match outside frame 2: the record alone
        if (tid == 0) {
            o.status = PSLFE_E_INVALID;
            *res = o;
        }
        return;
    }
    for (int i = tid; i < n1; i += PSL_INIT_BS) {
        p3d[3 * (size_t)i] = 0.f; p3d[3 * (size_t)i + 1] = 0.f; p3d[3 * (size_t)i + 2] = 0.f;
        tri[i] = 0;
        if (mout) mout[i] = matches[i];
    }
    if (tid == 0) {
        o.nmatches = N;
        o.best_it_h = o.best_it_f = o.best_hypothesis = -1;
    }
    if (N < 8) {   // uniform
        if (tid == 0) *res = o;
        return;
    }
    const PslInitRows R = {s_rows, N < PSL_INIT_LDS_ROWS ? N : PSL_INIT_LDS_ROWS, row_i, matches, k1, k2, A.ks};
    if (tid < 4) {
        const float* k = tid < 2 ? k1 : k2;
        const int n = tid < 2 ? n1 : n2;
        PslInitNorm* nm = tid < 2 ? &sh.nm1 : &sh.nm2;
        psl_init_normalize(k, A.ks, n, tid & 1, (tid & 1) ? &nm->my : &nm->mx, (tid & 1) ? &nm->sy : &nm->sx);
    }
    if (tid == 64) psl_rs_srand(&sh.rand, A.seed0 + (uint32_t)p);
    const float invS2 = psl_init_inv_sigma2(A.sigma);
    float SH = 0.f, SF = 0.f;   // thread 0's
    __syncthreads();
    for (int it0 = 0; it0 < A.max_its; it0 += PSL_INIT_B) {   // uniform
        const int nb = A.max_its - it0 < PSL_INIT_B ? A.max_its - it0 : PSL_INIT_B;
        if (tid == 64)
            for (int h = 0; h < nb; ++h) psl_rs_draw<8>(&sh.rand, N, sh.idx[h]);
        __syncthreads();
        if ((tid & 7) == 0) {
            const int f = tid >> 7, h = (tid & 127) >> 3;   // waves 0-1: H, waves 2-3: F
            if (h < nb) {
                const int s = f * PSL_INIT_B + h;
                if (!f) psl_init_hyp_h<2 * PSL_INIT_B>(&R, sh.idx[h], &sh.nm1, &sh.nm2, s_ws + s, s_wd + s, sh.model[h], sh.model[h] + 9);
                else psl_init_hyp_f<2 * PSL_INIT_B>(&R, sh.idx[h], &sh.nm1, &sh.nm2, s_ws + s, s_wd + s, sh.model[h] + 18);
            }
        }
        __syncthreads();
        if ((tid & 127) < nb) {   // lanes 0..nb-1 of waves 0 (H) and 2 (F)
            const int f = tid >> 7, h = tid & 127;
            float M[18], sc = 0.f;
#pragma unroll
            for (int k = 0; k < 18; ++k) M[k] = (f && k >= 9) ? 0.f : sh.model[h][(f ? 18 : 0) + k];
            for (int r = 0; r < N; ++r) {
                float q[4];
                psl_init_load(&R, r, q);
                if (!f) psl_init_score_h(M, M + 9, q, invS2, &sc);
                else psl_init_score_f(M, q, invS2, &sc);
            }
            sh.score[f][h] = sc;
        }
        __syncthreads();
        if (tid == 0)
            for (int h = 0; h < nb; ++h) {   // :165-170, :216-221
                if (sh.score[0][h] > SH) {
                    SH = sh.score[0][h]; o.best_it_h = it0 + h;
                    for (int k = 0; k < 18; ++k) sh.best[k] = sh.model[h][k];
                }
                if (sh.score[1][h] > SF) {
                    SF = sh.score[1][h]; o.best_it_f = it0 + h;
                    for (int k = 0; k < 9; ++k) sh.best[18 + k] = sh.model[h][18 + k];
                }
            }
        __syncthreads();
    }
    // the winners' flags, counted; RH, the branch, the motion hypotheses
    if (tid == 0) { sh.ok = o.best_it_h; sh.best_h = o.best_it_f; }
    __syncthreads();
    const int have_h = sh.ok >= 0, have_f = sh.best_h >= 0;
    __syncthreads();
    int ch = 0, cf = 0;
    for (int r0 = 0; r0 < N; r0 += PSL_INIT_BS) {   // uniform
        const int r = r0 + tid;
        int ih = 0, jf = 0;
        if (r < N) {
            float q[4];
            psl_init_load(&R, r, q);
            ih = have_h && psl_init_inlier(1, sh.best, q, invS2);
            jf = have_f && psl_init_inlier(0, sh.best + 18, q, invS2);
        }
        ch += __popcll(__ballot(ih));
        cf += __popcll(__ballot(jf));
    }
    if (lane == 0) { sh.part[wave] = ch; sh.cnt[wave] = cf; }
    __syncthreads();
    const int inl_h = sh.part[0] + sh.part[1] + sh.part[2] + sh.part[3], inl_f = sh.cnt[0] + sh.cnt[1] + sh.cnt[2] + sh.cnt[3];
    __syncthreads();
    float K[9];
    psl_init_K(&A.cam, K);
    if (tid == 0) {
        o.SH = SH; o.SF = SF; o.inliers_h = inl_h; o.inliers_f = inl_f;
        for (int k = 0; k < 9; ++k) { o.H21[k] = have_h ? sh.best[k] : 0.f; o.F21[k] = have_f ? sh.best[18 + k] : 0.f; }
        int nh = 0, hom = 0;
        if (!have_h && !have_f) {
            o.status = 4;
        } else {
            o.RH = PSL_RS_FDIV(SH, SH + SF);
            hom = (double)o.RH > 0.40;
            if (hom) {
                o.status |= 2;
                nh = psl_init_motion_h<1>(sh.best, K, s_ws, s_wd, s_ws + 9, sh.Rs, sh.ts) ? 8 : 0;
            } else {
                psl_init_motion_f<1>(sh.best + 18, K, s_ws, s_wd, s_ws + 9, sh.Rs, sh.ts);
                nh = 4;
            }
        }
        sh.nh = nh; sh.ok = hom;
    }
    __syncthreads();
    const int nh = sh.nh, homography = sh.ok;
    const float th2 = psl_init_th2(A.sigma);
    for (int h = 0; h < nh; ++h) {   // uniform
        if (tid == 0) psl_init_rt_setup(sh.Rs + 9 * h, sh.ts + 3 * h, K, th2, &sh.rt);
        __syncthreads();
        float par;
        const int g = init_check_rt(sh, s_ws, s_wd, R, N, homography, invS2, keys, false, p3d, tri, &par, nullptr);
        if (tid == 0) { o.ngood[h] = g; o.parallax[h] = par; }
    }
    if (tid == 0) {
        int best = -1, ok = 0;
        if (nh) ok = homography ? psl_init_decide_h(o.ngood, o.parallax, inl_h, 1.0f, 50, &best) : psl_init_decide_f(o.ngood, o.parallax, inl_f, 1.0f, 50, &best);
        o.best_hypothesis = best;
        sh.ok = ok; sh.best_h = best;
        if (ok) psl_init_rt_setup(sh.Rs + 9 * best, sh.ts + 3 * best, K, th2, &sh.rt);
    }
    __syncthreads();
    if (sh.ok) {   // uniform: the accepted hypothesis once more, writing vP3D and vbTriangulated (:527-531, :723-726)
        float par;
        int ntri = 0;
        init_check_rt(sh, s_ws, s_wd, R, N, homography, invS2, keys, true, p3d, tri, &par, &ntri);
        if (mout)   // src/Tracking.cc:712-719
            for (int i = tid; i < n1; i += PSL_INIT_BS)
                if (matches[i] >= 0 && !tri[i]) mout[i] = -1;
        if (tid == 0) {
            o.status |= 1;
            o.ntriangulated = ntri;
            for (int k = 0; k < 9; ++k) o.R21[k] = sh.Rs[9 * sh.best_h + k];
            for (int k = 0; k < 3; ++k) o.t21[k] = sh.ts[3 * sh.best_h + k];
        }
    }
    if (tid == 0) *res = o;
}

// the selection alone, for the tests: cosines [n] -> their keys, the selected cosine and its parallax
__global__ __launch_bounds__(PSL_INIT_BS) void k_init_debug_select(const float* cosines, int n, uint32_t* keys, float* out) {
    __shared__ InitShared sh;
    for (int j = threadIdx.x; j < n; j += PSL_INIT_BS) keys[j] = psl_init_cos_key(cosines[j]);
    __threadfence_block();
    __syncthreads();
    const float c = psl_init_cos_unkey(init_select_key(sh, keys, n));
    if (threadIdx.x == 0) { out[0] = c; out[1] = psl_init_parallax(c); }
}

namespace {

int init_check(const char* who, int npairs, int kstride, int mstride, int key_stride_bytes, float sigma, int max_its) {
    PSL_REQUIRE(npairs >= 0 && kstride >= 0 && mstride >= 0, PSLFE_E_INVALID, "%s: npairs = %d, kstride = %d, mstride = %d", who, npairs, kstride,
                mstride);
    PSL_REQUIRE(max_its >= 1, PSLFE_E_INVALID, "%s: max_its = %d", who, max_its);
    PSL_REQUIRE(sigma == sigma, PSLFE_E_INVALID, "%s: NaN sigma", who);
    PSL_REQUIRE(key_stride_bytes >= 8 && key_stride_bytes % 4 == 0, PSLFE_E_INVALID, "%s: key_stride_bytes = %d", who, key_stride_bytes);
    return PSLFE_OK;
}

// the caller has called psl_scratch_begin
int init_launch(pslfe_ctx* ctx, const char* who, InitArgs& A, int npairs) {
    const size_t n = (size_t)npairs * (size_t)A.mstride;
    A.row_i = static_cast<int32_t*>(psl_scratch(ctx, n ? n * sizeof(int32_t) : 1));
    A.cos_keys = static_cast<uint32_t*>(psl_scratch(ctx, n ? n * sizeof(uint32_t) : 1));
    PSL_REQUIRE(A.row_i && A.cos_keys, PSLFE_E_HIP, "%s: scratch", who);
    {
        PSL_STAGE_BEGIN(ctx, "init.solve");
        k_init_solve<<<npairs, PSL_INIT_BS, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "init.solve");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // namespace

extern "C" {

int pslfe_init_sets(uint32_t seed, int N, int max_its, int32_t* sets) {
    static const char* who = "pslfe_init_sets";
    PSL_REQUIRE(N >= 8 && max_its >= 0 && sets, PSLFE_E_INVALID, "%s: N = %d, max_its = %d or NULL sets", who, N, max_its);
    PslRsRand G;
    psl_rs_srand(&G, seed);
    for (int it = 0; it < max_its; ++it) {
        int idx[8];
        psl_rs_draw<8>(&G, N, idx);
        for (int j = 0; j < 8; ++j) sets[8 * (size_t)it + j] = idx[j];
    }
    return PSLFE_OK;
}

int pslfe_init_initialize_device(pslfe_ctx* ctx, int npairs, const void* d_keys1, const int32_t* d_nkeys1, const void* d_keys2,
                                 const int32_t* d_nkeys2, int key_stride_bytes, int kstride, const int32_t* d_matches12, int mstride,
                                 const PslCamera* cam, float sigma, int max_its, uint32_t seed0, PslInitResult* d_res, float* d_p3d,
                                 uint8_t* d_triangulated, int32_t* d_matches12_out) {
    static const char* who = "pslfe_init_initialize_device";
    if (int rc = init_check(who, npairs, kstride, mstride, key_stride_bytes, sigma, max_its)) return rc;
    if (npairs == 0) return PSLFE_OK;
    PSL_REQUIRE(ctx && cam, PSLFE_E_INVALID, "%s: NULL context or camera", who);
    PSL_REQUIRE(d_nkeys1 && d_nkeys2 && d_res, PSLFE_E_INVALID, "%s: NULL array", who);
    PSL_REQUIRE(kstride == 0 || (d_keys1 && d_keys2), PSLFE_E_INVALID, "%s: NULL keypoints with kstride = %d", who, kstride);
    PSL_REQUIRE(mstride == 0 || (d_matches12 && d_p3d && d_triangulated), PSLFE_E_INVALID, "%s: NULL matches or outputs with mstride = %d", who,
                mstride);
    PSL_HIP(hipSetDevice(ctx->device));
    if (int rc = psl_scratch_begin(ctx)) return rc;
    InitArgs A;
    memset(&A, 0, sizeof(A));
    A.keys1 = static_cast<const float*>(d_keys1); A.keys2 = static_cast<const float*>(d_keys2);
    A.n1 = d_nkeys1; A.n2 = d_nkeys2;
    A.ks = (size_t)key_stride_bytes / 4; A.kpair1 = A.kpair2 = A.ks * (size_t)kstride;
    A.kstride1 = A.kstride2 = kstride;
    A.matches = d_matches12; A.mstride = mstride; A.cam = *cam; A.sigma = sigma; A.max_its = max_its; A.seed0 = seed0;
    A.res = d_res; A.p3d = d_p3d; A.tri = d_triangulated; A.mout = d_matches12_out;
    return init_launch(ctx, who, A, npairs);
}

int pslfe_init_initialize_frames_device(pslfe_frame* f1, const int32_t* slot1, pslfe_frame* f2, const int32_t* slot2, int npairs,
                                        const int32_t* d_matches12, int mstride, const PslCamera* cam, float sigma, int max_its,
                                        uint32_t seed0, PslInitResult* d_res, float* d_p3d, uint8_t* d_triangulated,
                                        int32_t* d_matches12_out) {
    static const char* who = "pslfe_init_initialize_frames_device";
    if (int rc = init_check(who, npairs, 0, mstride, (int)sizeof(PslKeyPoint), sigma, max_its)) return rc;
    if (npairs == 0) return PSLFE_OK;
    PSL_REQUIRE(f1 && f2 && slot1 && slot2 && cam && d_res, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(f1->ctx == f2->ctx, PSLFE_E_INVALID, "%s: the frame stores belong to different contexts", who);
    PSL_REQUIRE(mstride >= f1->cap, PSLFE_E_INVALID, "%s: mstride %d < F1 capacity %d", who, mstride, f1->cap);
    PSL_REQUIRE(d_matches12 && d_p3d && d_triangulated, PSLFE_E_INVALID, "%s: NULL matches or outputs", who);
    for (int p = 0; p < npairs; ++p) {
        PSL_REQUIRE(slot1[p] >= 0 && slot1[p] < f1->max_frames && f1->slot_set[slot1[p]], PSLFE_E_STATE, "%s: pair %d: F1 slot %d not set", who, p,
                    slot1[p]);
        PSL_REQUIRE(slot2[p] >= 0 && slot2[p] < f2->max_frames && f2->slot_set[slot2[p]], PSLFE_E_STATE, "%s: pair %d: F2 slot %d not set", who, p,
                    slot2[p]);
    }
    pslfe_ctx* ctx = f1->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipStream_t st = ctx->stream;
    hipError_t e = hipSuccess;
    InitArgs A;
    memset(&A, 0, sizeof(A));
    A.slot1 = psl_scratch_up(ctx, slot1, (size_t)npairs, st, &e);
    A.slot2 = psl_scratch_up(ctx, slot2, (size_t)npairs, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    // the slot tables are pageable host memory: the call returns once their copies have run (the solver stays queued)
    hipEvent_t copied = nullptr;
    PSL_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
    e = hipEventRecord(copied, st);
    A.keys1 = reinterpret_cast<const float*>(f1->S.kps); A.keys2 = reinterpret_cast<const float*>(f2->S.kps);
    A.meta1 = f1->S.meta; A.meta2 = f2->S.meta;
    A.ks = sizeof(PslKeyPoint) / 4; A.kpair1 = A.ks * (size_t)f1->cap; A.kpair2 = A.ks * (size_t)f2->cap;
    A.kstride1 = f1->cap; A.kstride2 = f2->cap;
    A.matches = d_matches12; A.mstride = mstride; A.cam = *cam; A.sigma = sigma; A.max_its = max_its; A.seed0 = seed0;
    A.res = d_res; A.p3d = d_p3d; A.tri = d_triangulated; A.mout = d_matches12_out;
    int rc = e == hipSuccess ? init_launch(ctx, who, A, npairs) : PSLFE_E_HIP;
    if (e != hipSuccess) pslfe_set_error("%s: hipEventRecord: %s", who, hipGetErrorString(e));
    const hipError_t e2 = hipEventSynchronize(copied);
    (void)hipEventDestroy(copied);
    if (rc) return rc;
    PSL_HIP(e2);
    return PSLFE_OK;
}

int pslfe_init_initialize(pslfe_ctx* ctx, const float* keys1, int n1, const float* keys2, int n2, const int32_t* matches12,
                          const PslCamera* cam, float sigma, int max_its, uint32_t seed, PslInitResult* res, float* p3d,
                          uint8_t* triangulated) {
    static const char* who = "pslfe_init_initialize";
    PSL_REQUIRE(n1 >= 0 && n2 >= 0, PSLFE_E_INVALID, "%s: n1 = %d, n2 = %d", who, n1, n2);
    if (int rc = init_check(who, 1, n1 > n2 ? n1 : n2, n1, 8, sigma, max_its)) return rc;
    PSL_REQUIRE(ctx && cam && res, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(n1 == 0 || (keys1 && matches12 && p3d && triangulated), PSLFE_E_INVALID, "%s: NULL array with n1 = %d", who, n1);
    PSL_REQUIRE(n2 == 0 || keys2, PSLFE_E_INVALID, "%s: NULL keys2 with n2 = %d", who, n2);
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int kstride = n1 > n2 ? n1 : n2;
    const int32_t c1 = n1, c2 = n2;
    float* d_k1 = psl_scratch_up(ctx, (const float*)nullptr, 2 * (size_t)kstride, st, &e);
    float* d_k2 = psl_scratch_up(ctx, (const float*)nullptr, 2 * (size_t)kstride, st, &e);
    if (e == hipSuccess && n1) e = hipMemcpyAsync(d_k1, keys1, 2 * (size_t)n1 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n2) e = hipMemcpyAsync(d_k2, keys2, 2 * (size_t)n2 * sizeof(float), hipMemcpyHostToDevice, st);
    const int32_t* d_n1 = psl_scratch_up(ctx, &c1, 1, st, &e);
    const int32_t* d_n2 = psl_scratch_up(ctx, &c2, 1, st, &e);
    const int32_t* d_m = psl_scratch_up(ctx, n1 ? matches12 : nullptr, (size_t)n1, st, &e);
    PslInitResult* d_res = psl_scratch_up(ctx, (const PslInitResult*)nullptr, 1, st, &e);
    float* d_p3d = psl_scratch_up(ctx, (const float*)nullptr, 3 * (size_t)n1, st, &e);
    uint8_t* d_tri = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)n1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    InitArgs A;
    memset(&A, 0, sizeof(A));
    A.keys1 = d_k1; A.keys2 = d_k2; A.n1 = d_n1; A.n2 = d_n2;
    A.ks = 2; A.kpair1 = A.kpair2 = 2 * (size_t)kstride; A.kstride1 = A.kstride2 = kstride;
    A.matches = d_m; A.mstride = n1; A.cam = *cam; A.sigma = sigma; A.max_its = max_its; A.seed0 = seed;
    A.res = d_res; A.p3d = d_p3d; A.tri = d_tri; A.mout = nullptr;
    if (int rc = init_launch(ctx, who, A, 1)) return rc;
    PSL_HIP(hipMemcpyAsync(res, d_res, sizeof(PslInitResult), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    if (res->status < 0) {   // no output byte of the pair was written
        pslfe_set_error("%s: status %d (a match outside frame 2)", who, res->status);
        return res->status;
    }
    if (n1) PSL_HIP(hipMemcpyAsync(p3d, d_p3d, 3 * (size_t)n1 * sizeof(float), hipMemcpyDeviceToHost, st));
    if (n1) PSL_HIP(hipMemcpyAsync(triangulated, d_tri, (size_t)n1, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_init_debug_select(pslfe_ctx* ctx, const float* cosines, int n, uint32_t* keys, float* selected, float* parallax) {
    static const char* who = "pslfe_init_debug_select";
    PSL_REQUIRE(ctx && cosines && keys && selected && parallax && n >= 1, PSLFE_E_INVALID, "%s: NULL argument or n = %d", who, n);
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const float* d_c = psl_scratch_up(ctx, cosines, (size_t)n, st, &e);
    uint32_t* d_k = psl_scratch_up(ctx, (const uint32_t*)nullptr, (size_t)n, st, &e);
    float* d_o = psl_scratch_up(ctx, (const float*)nullptr, 2, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    k_init_debug_select<<<1, PSL_INIT_BS, 0, st>>>(d_c, n, d_k, d_o);
    PSL_HIP(hipGetLastError());
    float o[2];
    PSL_HIP(hipMemcpyAsync(keys, d_k, (size_t)n * sizeof(uint32_t), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(o, d_o, sizeof(o), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    *selected = o[0]; *parallax = o[1];
    return PSLFE_OK;
}

}  // extern "C"
