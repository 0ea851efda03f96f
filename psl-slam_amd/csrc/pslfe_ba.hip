// libpslfe: the point edges of Optimizer::LocalBundleAdjustment (src/Optimizer.cc:1025-1966; the EdgeSE3ProjectXYZ /
// EdgeStereoSE3ProjectXYZ part of LocalBundleAdjustmentAndInseclines :1968-2534) for K problems in one launch.  Product code.
// Who owns what.  ba_kernels.h holds everything that is arithmetic or a decision: the edges, the quadratic form, the Schur
// complement, the LDLt, the `Problem` of the Levenberg driver psl_lm_levenberg (lm_kernels.h) and the two rounds, written once over
// an executor (the contract: lm_kernels.h); the host loop of tools/dropin/ba_main.cpp runs the same text on one core.  This file
// owns the handle, the two pre-pass kernels and the entry points; the executor of a workgroup is PslLmWorkgroup of lm_device.h.
// Conventions: include/pslfe.h above pslfe_ba_local_device.
//
// The kernels are templates over LIL, the switch of ba_kernels.h: pslfe_ba_local[_device] launch the <false> instantiations (the
// point-only text; 183 VGPRs, scratch 0, LDS 5184 B as before), pslfe_ba_local_lil[_device] the <true> ones, which also check, list
// and optimise the VertexLIL rows and the LIL edges of LocalBundleAdjustmentAndInseclines (:2250-2533; 248 VGPRs, scratch 0:
// profiles/local_ba_lil_codegen.txt).
//
// Launches.  k_ba_check (the offsets, the counts against the handle's caps, the rows an edge names) and k_ba_lists (the four edge
// lists by stable counting sorts, the duplicate pairs) write a status per problem; k_ba_local optimises the problems whose status
// is PSLFE_OK and copies the others through.  All three have one workgroup per problem; a problem's result depends on nothing but
// its own rows, so neither the batch size nor the position in the batch matters.
//
// k_ba_local: one resident workgroup of 256 threads per problem through both rounds, every iteration and every trial; there is no
// launch per iteration.  The executor spreads the indices of a step over the threads (lane = edge for errors and Jacobians; thread
// = (block, entry) walking that block's edge list in order for Hpp, Hll and S; thread = row for a column of the LDLt; thread = point
// for the back-substitution; thread = vertex for the candidates) and ends the step with a barrier; sum256 is the ordered reduction
// psl_lm_reduce of lm_device.h.  Control flow is uniform: every decision is taken from values all threads read back after a barrier.
//
// Workgroup size.  256 threads = 4 waves: the ordered reduction of lm_device.h is defined on 256 partial sums, and the result must
// not depend on the geometry, so the size is fixed.  The workspaces do not fit LDS (160 KB per workgroup on gfx950: S alone is 259
// KB at N = 180, the edge rows of 20 000 edges 7.5 MB), so they live in HBM / L2 (4 MB per XCD holds S, the lists and the hot edge
// rows of one problem per resident workgroup); LDS holds the 64 bytes of the reduction and 20 bytes per thread of small arrays the
// compiler keeps there (183 VGPRs, no scratch, 2 waves per SIMD: profiles/local_ba_codegen.txt).  The kernel is latency bound (dependent
// double-precision chains in the LDLt and the substitutions, ~2 N + 15 barriers per trial), not occupancy bound: a single problem
// uses one CU, and the device fills only when K reaches the CU count.  profiles/local_ba_bench.json has the first timings.
#include <string.h>

#include "pslfe_internal.h"
#include "ba_kernels.h"
#include "lm_device.h"

#define PSL_BA_BS PSL_LM_LANES

static_assert(sizeof(PslBaLilEdge) == 72 && sizeof(PslMapLil) == 128, "local BA LIL PODs");
static_assert(sizeof(PslBaEdge) == 24 && sizeof(PslBaKeyFrame) == 52 && sizeof(PslBaInfo) == 48 && sizeof(PslMapPointGeom) == 32, "local BA PODs");
static_assert(PSL_BA_BS == 4 * PSL_LM_GROUP, "four waves of 64");

__device__ const double g_ba_sctab[444] = {
#include "psl_sincostab.inc"
};

struct pslfe_ba {
    pslfe_ctx* ctx = nullptr;
    int max_problems = 0, ckf = 0, cmp = 0, ced = 0, clil = 0, cle = 0;
    size_t ws_stride = 0;
    PslDeviceBuffers bufs;
    char* d_ws = nullptr;          // [max_problems][ws_stride]
    int32_t* d_status = nullptr;   // [max_problems][2]: status, has work
    int32_t* d_lil0 = nullptr;     // LIL caps of 0: [max_problems][ckf + 2], the offsets of the (empty) LIL lists; the workspace then has
                                   // no LIL views and the layout and stride pslfe_ba_create always gave
};

struct BaArgs {
    const PslBaKeyFrame* kf;
    const int32_t* kf_off;
    const PslMapPointGeom* mp;
    const int32_t* mp_off;
    const PslBaEdge* ed;
    const int32_t* ed_off;
    PslPoseCamD K;
    int rounds, ckf, cmp, ced;
    char* ws;
    size_t ws_stride;
    int32_t* status;
    PslBaKeyFrame* kf_out;
    PslMapPointGeom* mp_out;
    uint8_t* erase;
    PslBaInfo* info;
    // the LILs (the <true> instantiations)
    const PslMapLil* lil;
    const int32_t* lil_off;
    const PslBaLilEdge* led;
    const int32_t* led_off;
    int clil, cle;
    int32_t* lil0;
    PslMapLil* lil_out;
    uint8_t* erase_lil;
    int32_t* nerased_lil;
};

// the rows of problem k and, when its counts fit the caps (*code == PSLFE_OK), the views of its workspace; 0 when its offsets name
// no rows at all
template <bool LIL>
__device__ static int ba_problem(const BaArgs& A, int k, PslBaWs* W, int* code) {
    const int k0 = A.kf_off[k], k1 = A.kf_off[k + 1], p0 = A.mp_off[k], p1 = A.mp_off[k + 1], e0 = A.ed_off[k], e1 = A.ed_off[k + 1];
    if (k0 < 0 || p0 < 0 || e0 < 0 || k1 < k0 || p1 < p0 || e1 < e0) { *code = PSLFE_E_INVALID; return 0; }
    if constexpr (LIL) {
        const int l0 = A.lil_off[k], l1 = A.lil_off[k + 1], f0 = A.led_off[k], f1 = A.led_off[k + 1];
        if (l0 < 0 || f0 < 0 || l1 < l0 || f1 < f0) { *code = PSLFE_E_INVALID; return 0; }
        W->lil = A.lil + l0; W->led = A.led + f0;
        W->nlil = l1 - l0; W->nle = f1 - f0;
    }
    W->kf = A.kf + k0; W->mp = A.mp + p0; W->ed = A.ed + e0;
    W->nkf = k1 - k0; W->nmp = p1 - p0; W->ne = e1 - e0;
    W->K = A.K;
    W->sctab = g_ba_sctab;
    if (k1 - k0 > A.ckf || p1 - p0 > A.cmp || e1 - e0 > A.ced) { *code = PSLFE_E_CAPACITY; return 1; }
    if constexpr (LIL) {
        if (W->nlil > A.clil || W->nle > A.cle) { *code = PSLFE_E_CAPACITY; return 1; }
        if (A.lil0) {   // no LIL fits: only the offsets of the empty lists are read
            psl_ba_carve(A.ws + (size_t)k * A.ws_stride, A.ckf, A.cmp, A.ced, W);
            W->lkoff = A.lil0 + (size_t)k * (A.ckf + 2);
            W->lloff = W->lkoff + A.ckf + 1;
        } else {
            psl_ba_carve(A.ws + (size_t)k * A.ws_stride, A.ckf, A.cmp, A.ced, W, A.clil, A.cle);
        }
    } else {
        psl_ba_carve(A.ws + (size_t)k * A.ws_stride, A.ckf, A.cmp, A.ced, W);
    }
    *code = PSLFE_OK;
    return 1;
}

// pre-pass 1: the rows.  status[2k] = the problem's code, status[2k + 1] = 1 when it has an edge and a free keyframe
template <bool LIL>
__global__ __launch_bounds__(PSL_BA_BS) void k_ba_check(BaArgs A) {
    __shared__ int s_bad, s_free;
    const int k = blockIdx.x, tid = threadIdx.x;
    PslBaWs W;
    int code;
    if (tid == 0) { s_bad = 0; s_free = 0; }
    __syncthreads();
    if (!ba_problem<LIL>(A, k, &W, &code) || code != PSLFE_OK) {   // uniform
        if (tid == 0) { A.status[2 * k] = code; A.status[2 * k + 1] = 0; }
        return;
    }
    if constexpr (LIL)
        for (int e = tid; e < W.nle; e += PSL_BA_BS) {
            const int l = W.led[e].lil, f = W.led[e].kf;
            if (f < 0 || f >= W.nkf || l < 0 || l >= W.nlil) s_bad = 1;
        }
    for (int e = tid; e < W.ne; e += PSL_BA_BS) {
        const PslBaEdge ed = W.ed[e];
        if (ed.kf < 0 || ed.kf >= W.nkf || ed.point < 0 || ed.point >= W.nmp) s_bad = 1;
    }
    for (int v = tid; v < W.nkf; v += PSL_BA_BS)
        if (!W.kf[v].fixed) s_free = 1;
    __syncthreads();
    if (tid == 0) {
        A.status[2 * k] = s_bad ? PSLFE_E_INVALID : PSLFE_OK;
        A.status[2 * k + 1] = !s_bad && s_free && (W.ne > 0 || (LIL && W.nle > 0));
    }
}

// a stable counting sort of the edges src[0..ne) (NULL: 0, 1, 2, ...) by key into dst, as psl_ba_sort_host: the edges in chunks of
// 256 in list order; inside a chunk an edge's place is its key's cursor plus the earlier edges of the chunk with the same key
// (key(e): the key of edge e; ne edges)
template <class Key>
__device__ static void ba_sort_by(const PslBaWs& W, int ne, Key key_of, const int32_t* src, int nkeys, int32_t* off, int32_t* dst, int* s_key) {
    const int tid = threadIdx.x;
    for (int k = tid; k <= nkeys; k += PSL_BA_BS) off[k] = 0;
    __syncthreads();
    for (int e = tid; e < ne; e += PSL_BA_BS) atomicAdd(&off[key_of(e) + 1], 1);
    __syncthreads();
    if (tid == 0)
        for (int k = 0; k < nkeys; ++k) off[k + 1] += off[k];
    __syncthreads();
    for (int k = tid; k < nkeys; k += PSL_BA_BS) W.cursor[k] = off[k];
    __syncthreads();
    for (int a0 = 0; a0 < ne; a0 += PSL_BA_BS) {   // uniform
        const int a = a0 + tid;
        const int e = a < ne ? (src ? src[a] : a) : -1;
        const int key = e >= 0 ? key_of(e) : -1;
        s_key[tid] = key;
        __syncthreads();
        int at = 0;
        if (e >= 0) {
            at = W.cursor[key];
            for (int t = 0; t < tid; ++t) at += s_key[t] == key;
        }
        __syncthreads();
        if (e >= 0) {
            dst[at] = e;
            atomicAdd(&W.cursor[key], 1);
        }
        __syncthreads();
    }
}

__device__ static void ba_sort(const PslBaWs& W, const int32_t* src, int by_point, int nkeys, int32_t* off, int32_t* dst, int* s_key) {
    if (by_point) ba_sort_by(W, W.ne, [&](int e) { return W.ed[e].point; }, src, nkeys, off, dst, s_key);
    else ba_sort_by(W, W.ne, [&](int e) { return W.ed[e].kf; }, src, nkeys, off, dst, s_key);
}
__device__ static void ba_sort_lil(const PslBaWs& W, const int32_t* src, int by_lil, int nkeys, int32_t* off, int32_t* dst, int* s_key) {
    if (by_lil) ba_sort_by(W, W.nle, [&](int e) { return W.led[e].lil; }, src, nkeys, off, dst, s_key);
    else ba_sort_by(W, W.nle, [&](int e) { return W.led[e].kf; }, src, nkeys, off, dst, s_key);
}

// pre-pass 2: the lists of a problem that passed the first and has work, and the duplicate (point, keyframe) pairs: neighbours in
// the (point, keyframe) list
template <bool LIL>
__global__ __launch_bounds__(PSL_BA_BS) void k_ba_lists(BaArgs A) {
    __shared__ int s_key[PSL_BA_BS];
    __shared__ int s_dup;
    const int k = blockIdx.x, tid = threadIdx.x;
    if (A.status[2 * k] != PSLFE_OK || !A.status[2 * k + 1]) return;   // uniform
    PslBaWs W;
    int code;
    ba_problem<LIL>(A, k, &W, &code);
    if (tid == 0) s_dup = 0;
    ba_sort(W, nullptr, 0, W.nkf, W.koff, W.klist, s_key);
    ba_sort(W, nullptr, 1, W.nmp, W.poff, W.plist, s_key);
    ba_sort(W, W.plist, 0, W.nkf, W.koff, W.kplist, s_key);
    ba_sort(W, W.klist, 1, W.nmp, W.poff, W.pklist, s_key);
    for (int a = 1 + tid; a < W.ne; a += PSL_BA_BS) {
        const PslBaEdge x = W.ed[W.pklist[a - 1]], y = W.ed[W.pklist[a]];
        if (x.point == y.point && x.kf == y.kf) s_dup = 1;
    }
    if constexpr (LIL) {
        ba_sort_lil(W, nullptr, 0, W.nkf, W.lkoff, W.lklist, s_key);
        ba_sort_lil(W, nullptr, 1, W.nlil, W.lloff, W.lllist, s_key);
        ba_sort_lil(W, W.lllist, 0, W.nkf, W.lkoff, W.lkllist, s_key);
        ba_sort_lil(W, W.lklist, 1, W.nlil, W.lloff, W.llklist, s_key);
        for (int a = 1 + tid; a < W.nle; a += PSL_BA_BS) {
            const PslBaLilEdge x = W.led[W.llklist[a - 1]], y = W.led[W.llklist[a]];
            if (x.lil == y.lil && x.kf == y.kf) s_dup = 1;
        }
    }
    __syncthreads();
    if (tid == 0 && s_dup) A.status[2 * k] = PSLFE_E_INVALID;
}

template <bool LIL>
__global__ __launch_bounds__(PSL_BA_BS) void k_ba_local(BaArgs A) {
    __shared__ double s_red[2 * 4];
    const int k = blockIdx.x, tid = threadIdx.x;
    PslBaWs W;
    int code;
    const int have = ba_problem<LIL>(A, k, &W, &code);
    if (have && code == PSLFE_OK) code = A.status[2 * k];   // what the pre-passes found in the rows
    const int work = have && code == PSLFE_OK && A.status[2 * k + 1];
    uint8_t* erase = nullptr;
    if (have) erase = A.erase + A.ed_off[k];
    if (!work) {   // uniform: the outputs are the inputs
        if (have) {
            PslBaKeyFrame* ko = A.kf_out + A.kf_off[k];
            PslMapPointGeom* po = A.mp_out + A.mp_off[k];
            for (int v = tid; v < W.nkf; v += PSL_BA_BS) { const PslBaKeyFrame t = W.kf[v]; ko[v] = t; }
            for (int p = tid; p < W.nmp; p += PSL_BA_BS) { const PslMapPointGeom t = W.mp[p]; po[p] = t; }
            for (int e = tid; e < W.ne; e += PSL_BA_BS) erase[e] = 0;
            if constexpr (LIL) {
                PslMapLil* lo = A.lil_out + A.lil_off[k];
                uint8_t* el = A.erase_lil + A.led_off[k];
                for (int j = tid; j < W.nlil; j += PSL_BA_BS) { const PslMapLil t = W.lil[j]; lo[j] = t; }
                for (int e = tid; e < W.nle; e += PSL_BA_BS) el[e] = 0;
            }
        }
        if constexpr (LIL)
            if (tid == 0 && A.nerased_lil) A.nerased_lil[k] = 0;
        if (tid == 0) {
            PslBaInfo I;
            I.status = code; I.rounds = 0; I.iterations[0] = 0; I.iterations[1] = 0; I.nerased = 0;
            I.chi2_start = 0.0; I.chi2_round1 = 0.0; I.chi2_end = 0.0;
            A.info[k] = I;
        }
        return;
    }
    PslLmWorkgroup X = {s_red, 0};
    if constexpr (LIL)
        psl_ba_rounds<true>(X, W, A.rounds, A.kf_out + A.kf_off[k], A.mp_out + A.mp_off[k], erase, A.info + k, A.lil_out + A.lil_off[k],
                            A.erase_lil + A.led_off[k], A.nerased_lil ? A.nerased_lil + k : nullptr);
    else
        psl_ba_rounds(X, W, A.rounds, A.kf_out + A.kf_off[k], A.mp_out + A.mp_off[k], erase, A.info + k);
}

static int ba_create(const char* who, pslfe_ctx* ctx, int max_problems, int max_keyframes, int max_points, int max_edges, int max_lils,
                     int max_lil_edges, pslfe_ba** out) {
    PSL_REQUIRE(ctx && out, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(max_lils >= 0 && max_lil_edges >= 0, PSLFE_E_INVALID, "%s: max_lils = %d, max_lil_edges = %d", who, max_lils, max_lil_edges);
    PSL_REQUIRE(max_problems >= 1 && max_keyframes >= 1 && max_points >= 1 && max_edges >= 1, PSLFE_E_INVALID,
                "%s: max_problems = %d, max_keyframes = %d, max_points = %d, max_edges = %d", who, max_problems, max_keyframes, max_points,
                max_edges);
    PSL_REQUIRE(max_keyframes <= 4096, PSLFE_E_INVALID, "%s: max_keyframes = %d (S has 36 max_keyframes^2 doubles per problem)", who, max_keyframes);
    PSL_HIP(hipSetDevice(ctx->device));
    pslfe_ba* b = new pslfe_ba;
    b->ctx = ctx; b->max_problems = max_problems; b->ckf = max_keyframes; b->cmp = max_points; b->ced = max_edges;
    b->clil = max_lils; b->cle = max_lil_edges;
    PslBaWs W;
    const bool lils = max_lils > 0 || max_lil_edges > 0;
    b->ws_stride = psl_align_up(lils ? psl_ba_carve(nullptr, max_keyframes, max_points, max_edges, &W, max_lils, max_lil_edges)
                                     : psl_ba_carve(nullptr, max_keyframes, max_points, max_edges, &W), 256);
    b->bufs.alloc(b->d_ws, b->ws_stride * (size_t)max_problems, "workspaces");
    if (!lils) b->bufs.alloc(b->d_lil0, ((size_t)max_keyframes + 2) * (size_t)max_problems, "empty LIL lists");
    b->bufs.alloc(b->d_status, 2 * (size_t)max_problems, "status");
    if (int rc = b->bufs.check(who)) { delete b; return rc; }
    *out = b;
    return PSLFE_OK;
}

// the three launches of a call
template <bool LIL>
static int ba_launch(pslfe_ctx* ctx, int K, const BaArgs& A) {
    {
        PSL_STAGE_BEGIN(ctx, "ba.check");
        k_ba_check<LIL><<<K, PSL_BA_BS, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "ba.check");
    }
    {
        PSL_STAGE_BEGIN(ctx, "ba.lists");
        k_ba_lists<LIL><<<K, PSL_BA_BS, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "ba.lists");
    }
    {
        PSL_STAGE_BEGIN(ctx, "ba.local");
        k_ba_local<LIL><<<K, PSL_BA_BS, 0, ctx->stream>>>(A);
        PSL_STAGE_END(ctx, "ba.local");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

extern "C" {

int pslfe_ba_create(pslfe_ctx* ctx, int max_problems, int max_keyframes, int max_points, int max_edges, pslfe_ba** out) {
    return ba_create("pslfe_ba_create", ctx, max_problems, max_keyframes, max_points, max_edges, 0, 0, out);
}

int pslfe_ba_create_lil(pslfe_ctx* ctx, int max_problems, int max_keyframes, int max_points, int max_edges, int max_lils, int max_lil_edges,
                        pslfe_ba** out) {
    return ba_create("pslfe_ba_create_lil", ctx, max_problems, max_keyframes, max_points, max_edges, max_lils, max_lil_edges, out);
}

void pslfe_ba_destroy(pslfe_ba* ba) {
    if (!ba) return;
    (void)hipSetDevice(ba->ctx->device);
    (void)hipStreamSynchronize(ba->ctx->stream);
    delete ba;
}

int pslfe_ba_local_device(pslfe_ba* ba, int K, const PslBaKeyFrame* d_kf, const int32_t* d_kf_off, const PslMapPointGeom* d_mp,
                          const int32_t* d_mp_off, const PslBaEdge* d_edges, const int32_t* d_edge_off, const PslCamera* cam, int rounds,
                          PslBaKeyFrame* d_kf_out, PslMapPointGeom* d_mp_out, uint8_t* d_erase, PslBaInfo* d_info) {
    static const char* who = "pslfe_ba_local_device";
    PSL_REQUIRE(K >= 0 && rounds >= 1 && rounds <= 2, PSLFE_E_INVALID, "%s: K = %d, rounds = %d (1..2)", who, K, rounds);
    if (K == 0) return PSLFE_OK;
    PSL_REQUIRE(ba && cam, PSLFE_E_INVALID, "%s: NULL handle or camera", who);
    PSL_REQUIRE(K <= ba->max_problems, PSLFE_E_INVALID, "%s: K = %d above max_problems = %d", who, K, ba->max_problems);
    PSL_REQUIRE(d_kf && d_kf_off && d_mp && d_mp_off && d_edges && d_edge_off && d_kf_out && d_mp_out && d_erase && d_info, PSLFE_E_INVALID,
                "%s: NULL array", who);
    pslfe_ctx* ctx = ba->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    BaArgs A = {};
    A.kf = d_kf; A.kf_off = d_kf_off; A.mp = d_mp; A.mp_off = d_mp_off; A.ed = d_edges; A.ed_off = d_edge_off;
    A.K.fx = (double)cam->fx; A.K.fy = (double)cam->fy; A.K.cx = (double)cam->cx; A.K.cy = (double)cam->cy; A.K.bf = (double)cam->bf;
    A.rounds = rounds; A.ckf = ba->ckf; A.cmp = ba->cmp; A.ced = ba->ced;
    A.ws = ba->d_ws; A.ws_stride = ba->ws_stride; A.status = ba->d_status;
    A.kf_out = d_kf_out; A.mp_out = d_mp_out; A.erase = d_erase; A.info = d_info;
    A.clil = ba->clil; A.cle = ba->cle;   // the workspace's layout
    return ba_launch<false>(ctx, K, A);
}

int pslfe_ba_local_lil_device(pslfe_ba* ba, int K, const PslBaKeyFrame* d_kf, const int32_t* d_kf_off, const PslMapPointGeom* d_mp,
                              const int32_t* d_mp_off, const PslBaEdge* d_edges, const int32_t* d_edge_off, const PslMapLil* d_lil,
                              const int32_t* d_lil_off, const PslBaLilEdge* d_lil_edges, const int32_t* d_lil_edge_off, const PslCamera* cam,
                              int rounds, PslBaKeyFrame* d_kf_out, PslMapPointGeom* d_mp_out, uint8_t* d_erase, PslMapLil* d_lil_out,
                              uint8_t* d_erase_lil, int32_t* d_nerased_lil, PslBaInfo* d_info) {
    static const char* who = "pslfe_ba_local_lil_device";
    PSL_REQUIRE(K >= 0 && rounds >= 1 && rounds <= 2, PSLFE_E_INVALID, "%s: K = %d, rounds = %d (1..2)", who, K, rounds);
    if (K == 0) return PSLFE_OK;
    PSL_REQUIRE(ba && cam, PSLFE_E_INVALID, "%s: NULL handle or camera", who);
    PSL_REQUIRE(K <= ba->max_problems, PSLFE_E_INVALID, "%s: K = %d above max_problems = %d", who, K, ba->max_problems);
    PSL_REQUIRE(d_kf && d_kf_off && d_mp && d_mp_off && d_edges && d_edge_off && d_kf_out && d_mp_out && d_erase && d_info && d_lil && d_lil_off &&
                    d_lil_edges && d_lil_edge_off && d_lil_out && d_erase_lil,
                PSLFE_E_INVALID, "%s: NULL array", who);
    pslfe_ctx* ctx = ba->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    BaArgs A = {};
    A.kf = d_kf; A.kf_off = d_kf_off; A.mp = d_mp; A.mp_off = d_mp_off; A.ed = d_edges; A.ed_off = d_edge_off;
    A.K.fx = (double)cam->fx; A.K.fy = (double)cam->fy; A.K.cx = (double)cam->cx; A.K.cy = (double)cam->cy; A.K.bf = (double)cam->bf;
    A.rounds = rounds; A.ckf = ba->ckf; A.cmp = ba->cmp; A.ced = ba->ced;
    A.ws = ba->d_ws; A.ws_stride = ba->ws_stride; A.status = ba->d_status;
    A.kf_out = d_kf_out; A.mp_out = d_mp_out; A.erase = d_erase; A.info = d_info;
    A.lil = d_lil; A.lil_off = d_lil_off; A.led = d_lil_edges; A.led_off = d_lil_edge_off; A.clil = ba->clil; A.cle = ba->cle; A.lil0 = ba->d_lil0;
    A.lil_out = d_lil_out; A.erase_lil = d_erase_lil; A.nerased_lil = d_nerased_lil;
    return ba_launch<true>(ctx, K, A);
}

int pslfe_ba_local(pslfe_ba* ba, const PslBaKeyFrame* kf, int nkf, const PslMapPointGeom* mp, int nmp, const PslBaEdge* edges, int nedges,
                   const PslCamera* cam, int rounds, PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out, uint8_t* erase, PslBaInfo* info) {
    static const char* who = "pslfe_ba_local";
    PSL_REQUIRE(nkf >= 0 && nmp >= 0 && nedges >= 0 && rounds >= 1 && rounds <= 2, PSLFE_E_INVALID,
                "%s: nkf = %d, nmp = %d, nedges = %d, rounds = %d (1..2)", who, nkf, nmp, nedges, rounds);
    PSL_REQUIRE(ba && cam && info, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE((nkf == 0 || (kf && kf_out)) && (nmp == 0 || (mp && mp_out)) && (nedges == 0 || (edges && erase)), PSLFE_E_INVALID,
                "%s: NULL array with a non-zero count", who);
    pslfe_ctx* ctx = ba->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int32_t koff[2] = {0, nkf}, poff[2] = {0, nmp}, eoff[2] = {0, nedges};
    PslBaKeyFrame* d_kf = psl_scratch_up(ctx, nkf ? kf : nullptr, (size_t)nkf, st, &e);
    PslMapPointGeom* d_mp = psl_scratch_up(ctx, nmp ? mp : nullptr, (size_t)nmp, st, &e);
    PslBaEdge* d_ed = psl_scratch_up(ctx, nedges ? edges : nullptr, (size_t)nedges, st, &e);
    const int32_t* d_koff = psl_scratch_up(ctx, koff, 2, st, &e);
    const int32_t* d_poff = psl_scratch_up(ctx, poff, 2, st, &e);
    const int32_t* d_eoff = psl_scratch_up(ctx, eoff, 2, st, &e);
    uint8_t* d_erase = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)nedges, st, &e);
    PslBaInfo* d_info = psl_scratch_up(ctx, (const PslBaInfo*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    if (int rc = pslfe_ba_local_device(ba, 1, d_kf, d_koff, d_mp, d_poff, d_ed, d_eoff, cam, rounds, d_kf, d_mp, d_erase, d_info)) return rc;
    if (nkf) PSL_HIP(hipMemcpyAsync(kf_out, d_kf, (size_t)nkf * sizeof(PslBaKeyFrame), hipMemcpyDeviceToHost, st));
    if (nmp) PSL_HIP(hipMemcpyAsync(mp_out, d_mp, (size_t)nmp * sizeof(PslMapPointGeom), hipMemcpyDeviceToHost, st));
    if (nedges) PSL_HIP(hipMemcpyAsync(erase, d_erase, (size_t)nedges, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(info, d_info, sizeof(PslBaInfo), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    if (info->status < 0) {
        pslfe_set_error("%s: the problem was refused with %d (%s)", who, info->status,
                        info->status == PSLFE_E_CAPACITY ? "a count above the handle's caps" : "an edge outside the problem or a duplicate pair");
        return info->status;
    }
    return PSLFE_OK;
}

int pslfe_ba_local_lil(pslfe_ba* ba, const PslBaKeyFrame* kf, int nkf, const PslMapPointGeom* mp, int nmp, const PslBaEdge* edges, int nedges,
                       const PslMapLil* lil, int nlil, const PslBaLilEdge* lil_edges, int nlil_edges, const PslCamera* cam, int rounds,
                       PslBaKeyFrame* kf_out, PslMapPointGeom* mp_out, uint8_t* erase, PslMapLil* lil_out, uint8_t* erase_lil, PslBaInfo* info) {
    static const char* who = "pslfe_ba_local_lil";
    PSL_REQUIRE(nkf >= 0 && nmp >= 0 && nedges >= 0 && nlil >= 0 && nlil_edges >= 0 && rounds >= 1 && rounds <= 2, PSLFE_E_INVALID,
                "%s: nkf = %d, nmp = %d, nedges = %d, nlil = %d, nlil_edges = %d, rounds = %d (1..2)", who, nkf, nmp, nedges, nlil, nlil_edges, rounds);
    PSL_REQUIRE(ba && cam && info, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE((nkf == 0 || (kf && kf_out)) && (nmp == 0 || (mp && mp_out)) && (nedges == 0 || (edges && erase)) && (nlil == 0 || (lil && lil_out)) &&
                    (nlil_edges == 0 || (lil_edges && erase_lil)),
                PSLFE_E_INVALID, "%s: NULL array with a non-zero count", who);
    pslfe_ctx* ctx = ba->ctx;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    const int32_t koff[2] = {0, nkf}, poff[2] = {0, nmp}, eoff[2] = {0, nedges}, loff[2] = {0, nlil}, foff[2] = {0, nlil_edges};
    // a zero count still gets one row of scratch: the device form takes no NULL array
    PslBaKeyFrame* d_kf = psl_scratch_up(ctx, nkf ? kf : nullptr, (size_t)(nkf ? nkf : 1), st, &e);
    PslMapPointGeom* d_mp = psl_scratch_up(ctx, nmp ? mp : nullptr, (size_t)(nmp ? nmp : 1), st, &e);
    PslBaEdge* d_ed = psl_scratch_up(ctx, nedges ? edges : nullptr, (size_t)(nedges ? nedges : 1), st, &e);
    PslMapLil* d_lil = psl_scratch_up(ctx, nlil ? lil : nullptr, (size_t)(nlil ? nlil : 1), st, &e);
    PslBaLilEdge* d_led = psl_scratch_up(ctx, nlil_edges ? lil_edges : nullptr, (size_t)(nlil_edges ? nlil_edges : 1), st, &e);
    const int32_t* d_koff = psl_scratch_up(ctx, koff, 2, st, &e);
    const int32_t* d_poff = psl_scratch_up(ctx, poff, 2, st, &e);
    const int32_t* d_eoff = psl_scratch_up(ctx, eoff, 2, st, &e);
    const int32_t* d_loff = psl_scratch_up(ctx, loff, 2, st, &e);
    const int32_t* d_foff = psl_scratch_up(ctx, foff, 2, st, &e);
    uint8_t* d_erase = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)(nedges ? nedges : 1), st, &e);
    uint8_t* d_erase_lil = psl_scratch_up(ctx, (const uint8_t*)nullptr, (size_t)(nlil_edges ? nlil_edges : 1), st, &e);
    PslBaInfo* d_info = psl_scratch_up(ctx, (const PslBaInfo*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch / upload: %s", who, hipGetErrorString(e));
    if (int rc = pslfe_ba_local_lil_device(ba, 1, d_kf, d_koff, d_mp, d_poff, d_ed, d_eoff, d_lil, d_loff, d_led, d_foff, cam, rounds, d_kf, d_mp,
                                           d_erase, d_lil, d_erase_lil, nullptr, d_info))
        return rc;
    if (nkf) PSL_HIP(hipMemcpyAsync(kf_out, d_kf, (size_t)nkf * sizeof(PslBaKeyFrame), hipMemcpyDeviceToHost, st));
    if (nmp) PSL_HIP(hipMemcpyAsync(mp_out, d_mp, (size_t)nmp * sizeof(PslMapPointGeom), hipMemcpyDeviceToHost, st));
    if (nedges) PSL_HIP(hipMemcpyAsync(erase, d_erase, (size_t)nedges, hipMemcpyDeviceToHost, st));
    if (nlil) PSL_HIP(hipMemcpyAsync(lil_out, d_lil, (size_t)nlil * sizeof(PslMapLil), hipMemcpyDeviceToHost, st));
    if (nlil_edges) PSL_HIP(hipMemcpyAsync(erase_lil, d_erase_lil, (size_t)nlil_edges, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(info, d_info, sizeof(PslBaInfo), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    if (info->status < 0) {
        pslfe_set_error("%s: the problem was refused with %d (%s)", who, info->status,
                        info->status == PSLFE_E_CAPACITY ? "a count above the handle's caps" : "an edge outside the problem or a duplicate pair");
        return info->status;
    }
    return PSLFE_OK;
}

}  // extern "C"
