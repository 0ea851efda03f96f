// libpslfe: ORBmatcher::SearchForInitialization on the device (the monocular initialiser's matcher). Product code.
// Reference behaviour reproduced:
//   ORBmatcher::SearchForInitialization(F1, F2, vbPrevMatched, vnMatches12, windowSize)   src/ORBmatcher.cc:405-520
//   Frame::GetFeaturesInArea(x, y, r, 0, 0)                                             src/Frame.cc:985-1038
//   ORBmatcher::ComputeThreeMaxima                                                     src/ORBmatcher.cc:1601-1645
//
// The reference walks F1's octave-0 keypoints in ascending order; a query skips every F2 keypoint whose vMatchedDistance is
// <= its distance (:442-443), and an accepted query takes its keypoint from an earlier one (:462-466), whose rotHist entry
// stays.  Every accept strictly lowers vMatchedDistance[i2], so what query i1 sees for i2 is the prefix minimum of the
// accepted distances of the earlier queries that chose i2, and the final owner of i2 is the last query that accepted it.
// Three kernels per launch:
//   k_mono_grid0    F2's grid reduced to its octave-0 keypoints, per pair (the window's level band is octave 0 exactly; the
//                   reduction keeps the CSR order, so candidate positions still follow GetFeaturesInArea's visiting order);
//   k_mono_eval     one wave per F1 octave-0 keypoint of every pair: the PSL_MI_K smallest (distance, position) keys of its
//                   window, ascending, and whether the window holds more;
//   k_mono_resolve  one wave per pair walks the queries in order with vMatchedDistance / vnMatches21 in LDS: the first two
//                   cached keys that pass the distance filter are the best and the second best; a query whose list runs out
//                   while its window holds more re-walks the window in full.  Then the rotation histogram, ComputeThreeMaxima,
//                   the filter and the vbPrevMatched update.
#include <math.h>
#include <string.h>

#include <vector>

#include "pslfe_internal.h"
#include "psl_device_math.h"

#include "match_kernels.h"

#define PSL_MI_K 8       // cached candidates per query
#define PSL_MD_NONE 255  // vMatchedDistance == INT_MAX (every stored distance is <= TH_LOW)

struct MonoArgs {
    FrameStore S1, S2;
    const int* slot1;     // [npairs]
    const int* slot2;     // [npairs]
    float* prev;          // [pair][stride][2] vbPrevMatched
    int* matches12;       // [pair][stride]
    int* nmatches;        // [pair]
    int stride;
    float r;              // (float)windowSize
    float nnratio;
    int check_ori;
    int* gstart0;         // [pair][PSL_GRID_CELLS + 1] octave-0 grid of F2
    uint16_t* gidx0;      // [pair][S2.cap]
    uint32_t* topk;       // [pair][S1.cap][PSL_MI_K]: (dist << 16 | i2) in (dist, position) order, PSL_KEY_INF-terminated
    uint8_t* more;        // [pair][S1.cap]
};

// F2 of `pair`: its frame view and its octave-0 grid
struct MonoF2 {
    FrameView V;
    const int* gstart0;
    const uint16_t* gidx0;
};

__device__ __forceinline__ MonoF2 psl_mono_f2(const MonoArgs& A, int pair) {
    MonoF2 F;
    F.V = psl_frame_view(A.S2, A.slot2[pair]);
    F.gstart0 = A.gstart0 + (size_t)pair * (PSL_GRID_CELLS + 1);
    F.gidx0 = A.gidx0 + (size_t)pair * A.S2.cap;
    return F;
}

// Key (dist << 16 | position) of window candidate j, PSL_KEY_INF past the end, outside |dx| < r, |dy| < r, or - md != NULL -
// filtered by vMatchedDistance (:442-443).  Called by all 64 lanes.
__device__ __forceinline__ uint32_t psl_mono_key(const MonoF2& F, float x, float y, float r, const uint32_t (&qd)[8], const WindowCols& W, int j,
                                                 const uint8_t* md) {
    const int p = psl_window_pos(W, j);
    uint32_t key = PSL_KEY_INF;
    if (p >= 0) {
        const int i2 = F.gidx0[p];
        const float2 xy = *reinterpret_cast<const float2*>(&F.V.kps[i2].x);
        bool ok = __builtin_fabsf(PSL_FSUB(xy.x, x)) < r && __builtin_fabsf(PSL_FSUB(xy.y, y)) < r;
        const int dist = psl_hamming256(qd, F.V.desc + (size_t)i2 * 8);
        if (md) {
            const int m = md[i2];
            ok = ok && !(m != PSL_MD_NONE && m <= dist);
        }
        if (ok) key = ((uint32_t)dist << 16) | (uint32_t)p;
    }
    return key;
}

// ---------------------------------------------------------------------------------------------
// block = pair: F2's CSR grid without the keypoints of octave != 0.  Thread t owns cells 3t..3t+2 (as k_build_grid).
__global__ __launch_bounds__(1024) void k_mono_grid0(MonoArgs A) {
    __shared__ int s_w[17];
    const int pair = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const FrameView V = psl_frame_view(A.S2, A.slot2[pair]);
    int* gstart0 = A.gstart0 + (size_t)pair * (PSL_GRID_CELLS + 1);
    uint16_t* gidx0 = A.gidx0 + (size_t)pair * A.S2.cap;
    const int c0 = tid * 3;
    int cnt[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        cnt[k] = 0;
        for (int p = V.gstart[c0 + k]; p < V.gstart[c0 + k + 1]; ++p) {
            const int i = V.gidx[p];
            cnt[k] += (i < V.n && V.kps[i].octave == 0);
        }
    }
    int inc = cnt[0] + cnt[1] + cnt[2];
    const int mine = inc;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < 16; ++k) { const int t = s_w[k]; s_w[k] = acc; acc += t; }
        s_w[16] = acc;
    }
    __syncthreads();
    int w = inc - mine + s_w[wave];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        gstart0[c0 + k] = w;
        for (int p = V.gstart[c0 + k]; p < V.gstart[c0 + k + 1]; ++p) {
            const int i = V.gidx[p];
            if (i < V.n && V.kps[i].octave == 0) gidx0[w++] = (uint16_t)i;
        }
    }
    if (tid == 1023) gstart0[PSL_GRID_CELLS] = s_w[16];
}

// Pass 1 (wide): one wave per (F1 keypoint, pair).  Keypoints of octave > 0 and empty windows get an empty list.
__global__ __launch_bounds__(256) void k_mono_eval(MonoArgs A) {
    const int pair = blockIdx.y, qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const FrameView V1 = psl_frame_view(A.S1, A.slot1[pair]);
    if (qi >= V1.n) return;
    const size_t o = (size_t)pair * A.S1.cap + qi;
    uint32_t best = PSL_KEY_INF;  // lanes 0..PSL_MI_K-1: running smallest keys, ascending
    int cnt = 0;
    const MonoF2 F = psl_mono_f2(A, pair);
    if (V1.kps[qi].octave == 0) {  // level1 > 0 is skipped (:421-423)
        const float x = A.prev[((size_t)pair * A.stride + qi) * 2], y = A.prev[((size_t)pair * A.stride + qi) * 2 + 1];
        uint32_t qd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) qd[k] = V1.desc[(size_t)qi * 8 + k];
        // GetFeaturesInArea(x, y, r, 0, 0): the octave-0 grid makes the level band exact, checkLevels stays off
        const WindowCols W = psl_grid_cols(F.gstart0, F.V.M, x, y, A.r);
        for (int base = 0; base < W.T; base += 64) {
            const uint32_t key = psl_mono_key(F, x, y, A.r, qd, W, base + lane, nullptr);
            cnt += __popcll(__ballot(key != PSL_KEY_INF));
            best = psl_topk_merge<PSL_MI_K>(best, key, base == 0);
        }
    }
    if (lane < PSL_MI_K) {  // the position becomes the keypoint; the list keeps the (dist, position) order
        const uint32_t e = best == PSL_KEY_INF ? PSL_KEY_INF : ((best & 0xffff0000u) | (uint32_t)F.gidx0[best & 0xffff]);
        A.topk[o * PSL_MI_K + lane] = e;
    }
    if (lane == 0) A.more[o] = cnt > PSL_MI_K;
}

// Pass 2: one wave per pair, the reference's loop in order.
__global__ __launch_bounds__(64) void k_mono_resolve(MonoArgs A) {
    __shared__ uint8_t s_md[PSL_QMAX];   // vMatchedDistance, PSL_MD_NONE = INT_MAX
    __shared__ int16_t s_m21[PSL_QMAX];  // vnMatches21
    __shared__ int16_t s_acc[PSL_QMAX];  // keypoint the query accepted (| 0x4000 once taken by a later query), -1: none
    __shared__ uint8_t s_bin[PSL_QMAX];
    __shared__ int s_hist[PSL_HISTO];
    __shared__ int s_ind[3];
    const int pair = blockIdx.x, lane = threadIdx.x;
    const FrameView V1 = psl_frame_view(A.S1, A.slot1[pair]);
    const MonoF2 F = psl_mono_f2(A, pair);
    const int n1 = V1.n, n2 = F.V.n;
    for (int i = lane; i < n2; i += 64) { s_md[i] = PSL_MD_NONE; s_m21[i] = -1; }
    for (int i = lane; i < n1; i += 64) s_acc[i] = -1;
    if (lane < PSL_HISTO) s_hist[lane] = 0;
    __syncthreads();
    const uint32_t* TK = A.topk + (size_t)pair * A.S1.cap * PSL_MI_K;
    const uint8_t* MORE = A.more + (size_t)pair * A.S1.cap;
    const float* prev = A.prev + (size_t)pair * A.stride * 2;
    const int e = lane & (PSL_MI_K - 1);
    // eight queries' lists per round: lane 8k + e holds entry e of query base + k
    for (int base = 0; base < n1; base += 64 / PSL_MI_K) {
        const int qmine = base + (lane >> 3);
        const uint32_t ent = qmine < n1 ? TK[(size_t)qmine * PSL_MI_K + e] : PSL_KEY_INF;
        const int mflag = (qmine < n1 && e == 0) ? MORE[qmine] : 0;
        uint64_t active = __ballot(e == 0 && ent != PSL_KEY_INF);
        while (active) {
            const int src = __builtin_ctzll(active);
            active &= active - 1;
            const int qi = base + (src >> 3);
            const uint32_t my = __shfl(ent, (src & ~7) + e);
            int md = PSL_MD_NONE, i2 = 0, dist = 0;
            if (my != PSL_KEY_INF) { i2 = (int)(my & 0xffff); dist = (int)(my >> 16); md = s_md[i2]; }
            const bool surv = lane < PSL_MI_K && my != PSL_KEY_INF && !(md != PSL_MD_NONE && md <= dist);
            const uint32_t sm = (uint32_t)__ballot(surv);
            const int moreq = __shfl(mflag, src);
            int bestDist = 0x7fffffff, bestDist2 = 0x7fffffff, bestIdx2 = -1;
            if (__popc(sm) >= 2 || !moreq) {   // the list holds the two smallest survivors (or all of them)
                if (sm) {
                    const int e1 = __builtin_ctz(sm);
                    const uint32_t k1 = __shfl(my, e1);
                    bestDist = (int)(k1 >> 16); bestIdx2 = (int)(k1 & 0xffff);
                    const uint32_t rest = sm & (sm - 1);
                    if (rest) bestDist2 = (int)(__shfl(my, __builtin_ctz(rest)) >> 16);
                }
            } else {  // re-walk the window with the current vMatchedDistance
                const float x = prev[qi * 2], y = prev[qi * 2 + 1];
                uint32_t qd[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) qd[k] = V1.desc[(size_t)qi * 8 + k];
                const WindowCols W = psl_grid_cols(F.gstart0, F.V.M, x, y, A.r);
                uint32_t t0 = PSL_KEY_INF, t1 = PSL_KEY_INF;
                for (int b = 0; b < W.T; b += 64) {
                    const uint32_t key = psl_mono_key(F, x, y, A.r, qd, W, b + lane, s_md);
                    if (key < t0) { t1 = t0; t0 = key; } else if (key < t1) t1 = key;
                }
                psl_wave_min2(t0, t1);
                if (t0 != PSL_KEY_INF) { bestDist = (int)(t0 >> 16); bestIdx2 = F.gidx0[t0 & 0xffff]; }
                if (t1 != PSL_KEY_INF) bestDist2 = (int)(t1 >> 16);
            }
            // :457-468
            if (bestDist <= PSL_TH_LOW && (float)bestDist < PSL_FMUL((float)bestDist2, A.nnratio)) {
                if (lane == 0) {
                    const int old = s_m21[bestIdx2];
                    if (old >= 0) s_acc[old] = (int16_t)(s_acc[old] | 0x4000);
                    s_acc[qi] = (int16_t)bestIdx2;
                    s_m21[bestIdx2] = (int16_t)qi;
                    s_md[bestIdx2] = (uint8_t)bestDist;
                }
                __syncthreads();
            }
        }
    }
    __syncthreads();
    // rotation histogram (:470-481, :485-508): every accepted query counts, also one whose keypoint was taken later
    const bool ori = A.check_ori != 0;
    if (ori) {
        for (int qi = lane; qi < n1; qi += 64) {
            const int a = s_acc[qi];
            if (a < 0) continue;
            const int bin = psl_rot_bin(V1.kps[qi].angle, F.V.kps[a & 0xfff].angle);
            s_bin[qi] = (uint8_t)bin;
            atomicAdd(&s_hist[bin], 1);
        }
        __syncthreads();
        if (lane == 0) psl_three_maxima(s_hist, s_ind);
        __syncthreads();
    }
    // vnMatches12 and vbPrevMatched (:512-516)
    int* m12 = A.matches12 + (size_t)pair * A.stride;
    float* pv = A.prev + (size_t)pair * A.stride * 2;
    int local = 0;
    for (int qi = lane; qi < n1; qi += 64) {
        const int a = s_acc[qi];
        int m = (a >= 0 && !(a & 0x4000)) ? a : -1;
        if (m >= 0 && ori && !psl_rot_keep(s_bin[qi], s_ind)) m = -1;
        m12[qi] = m;
        if (m >= 0) {
            const float2 xy = *reinterpret_cast<const float2*>(&F.V.kps[m].x);
            pv[qi * 2] = xy.x; pv[qi * 2 + 1] = xy.y;
            ++local;
        }
    }
    local = psl_wave_sum(local);
    if (lane == 0) A.nmatches[pair] = local;
}

// ---------------------------------------------------------------------------------------------
namespace {
// slots checked by the caller; d_slot1 / d_slot2 in device memory; scratch begun by the caller
int mono_search(pslfe_frame* f1, const int* d_slot1, pslfe_frame* f2, const int* d_slot2, int npairs, float* d_prev, int stride, int window,
                float nnratio, int check_orientation, int32_t* d_matches12, int32_t* d_nmatches, const char* who) {
    pslfe_ctx* ctx = f1->ctx;
    MonoArgs A;
    memset(&A, 0, sizeof(A));
    A.S1 = f1->S; A.S2 = f2->S;
    A.slot1 = d_slot1; A.slot2 = d_slot2;
    A.prev = d_prev; A.matches12 = d_matches12; A.nmatches = d_nmatches; A.stride = stride;
    A.r = (float)window; A.nnratio = nnratio; A.check_ori = check_orientation;
    A.gstart0 = static_cast<int*>(psl_scratch(ctx, (size_t)npairs * (PSL_GRID_CELLS + 1) * sizeof(int)));
    A.gidx0 = static_cast<uint16_t*>(psl_scratch(ctx, (size_t)npairs * f2->cap * sizeof(uint16_t)));
    A.topk = static_cast<uint32_t*>(psl_scratch(ctx, (size_t)npairs * f1->cap * PSL_MI_K * sizeof(uint32_t)));
    A.more = static_cast<uint8_t*>(psl_scratch(ctx, (size_t)npairs * f1->cap));
    PSL_REQUIRE(A.gstart0 && A.gidx0 && A.topk && A.more, PSLFE_E_HIP, "%s: out of device memory", who);
    hipStream_t st = ctx->stream;
    {
        PSL_STAGE_BEGIN(ctx, "match.mono_init");
        k_mono_grid0<<<npairs, 1024, 0, st>>>(A);
        k_mono_eval<<<dim3((f1->cap + 3) / 4, npairs), 256, 0, st>>>(A);
        k_mono_resolve<<<npairs, 64, 0, st>>>(A);
        PSL_STAGE_END(ctx, "match.mono_init");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

int mono_check(pslfe_frame* f1, pslfe_frame* f2, int window, float nnratio, const char* who) {
    PSL_REQUIRE(f1->ctx == f2->ctx, PSLFE_E_INVALID, "%s: the frame stores belong to different contexts", who);
    PSL_REQUIRE(window >= 0, PSLFE_E_INVALID, "%s: window %d", who, window);
    PSL_REQUIRE(isfinite(nnratio), PSLFE_E_INVALID, "%s: nnratio is not finite", who);
    return PSLFE_OK;
}
}  // namespace

extern "C" {

int pslfe_orb_search_for_initialization_device(pslfe_frame* f1, const int32_t* slot1, pslfe_frame* f2, const int32_t* slot2, int npairs,
                                               float* d_prev, int prev_stride, int window, float nnratio, int check_orientation,
                                               int32_t* d_matches12, int32_t* d_nmatches) {
    const char* who = "pslfe_orb_search_for_initialization_device";
    PSL_REQUIRE(f1 && f2 && slot1 && slot2 && d_prev && d_matches12 && d_nmatches, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(npairs >= 1, PSLFE_E_INVALID, "%s: %d pairs", who, npairs);
    PSL_REQUIRE(prev_stride >= f1->cap, PSLFE_E_INVALID, "%s: prev_stride %d < F1 capacity %d", who, prev_stride, f1->cap);
    if (int rc = mono_check(f1, f2, window, nnratio, who)) return rc;
    for (int p = 0; p < npairs; ++p) {
        PSL_REQUIRE(slot1[p] >= 0 && slot1[p] < f1->max_frames && f1->slot_set[slot1[p]], PSLFE_E_STATE, "%s: pair %d: F1 slot %d not set", who, p,
                    slot1[p]);
        PSL_REQUIRE(slot2[p] >= 0 && slot2[p] < f2->max_frames && f2->slot_set[slot2[p]], PSLFE_E_STATE, "%s: pair %d: F2 slot %d not set", who, p,
                    slot2[p]);
    }
    PSL_HIP(hipSetDevice(f1->ctx->device));
    if (int rc = psl_scratch_begin(f1->ctx)) return rc;
    hipStream_t st = f1->ctx->stream;
    hipError_t e = hipSuccess;
    int* d_s1 = psl_scratch_up(f1->ctx, slot1, (size_t)npairs, st, &e);
    int* d_s2 = psl_scratch_up(f1->ctx, slot2, (size_t)npairs, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    // the slot tables are pageable host memory: the call returns once their copies have run (the matching stays queued)
    hipEvent_t copied = nullptr;
    PSL_HIP(hipEventCreateWithFlags(&copied, hipEventDisableTiming));
    e = hipEventRecord(copied, st);
    int rc = e == hipSuccess ? mono_search(f1, d_s1, f2, d_s2, npairs, d_prev, prev_stride, window, nnratio, check_orientation, d_matches12,
                                           d_nmatches, who)
                             : PSLFE_E_HIP;
    if (e != hipSuccess) pslfe_set_error("%s: hipEventRecord: %s", who, hipGetErrorString(e));
    const hipError_t e2 = hipEventSynchronize(copied);
    (void)hipEventDestroy(copied);
    if (rc) return rc;
    PSL_HIP(e2);
    return PSLFE_OK;
}

int pslfe_orb_search_for_initialization(pslfe_frame* f1, int slot1, pslfe_frame* f2, int slot2, float* prev_matched, int window, float nnratio,
                                        int check_orientation, int32_t* matches12, int* nmatches) {
    const char* who = "pslfe_orb_search_for_initialization";
    PSL_REQUIRE(f1 && f2 && nmatches, PSLFE_E_INVALID, "%s: NULL argument", who);
    if (int rc = mono_check(f1, f2, window, nnratio, who)) return rc;
    PSL_REQUIRE(slot1 >= 0 && slot1 < f1->max_frames && f1->slot_set[slot1], PSLFE_E_STATE, "%s: F1 slot %d not set", who, slot1);
    PSL_REQUIRE(slot2 >= 0 && slot2 < f2->max_frames && f2->slot_set[slot2], PSLFE_E_STATE, "%s: F2 slot %d not set", who, slot2);
    *nmatches = 0;
    PSL_HIP(hipSetDevice(f1->ctx->device));
    pslfe_ctx* ctx = f1->ctx;
    hipStream_t st = ctx->stream;
    FrameMeta m;
    char* hs = psl_host_stage(ctx, sizeof(m));
    PSL_REQUIRE(hs, PSLFE_E_HIP, "%s: no pinned staging memory (hipHostMalloc)", who);
    PSL_HIP(hipMemcpyAsync(hs, f1->S.meta + slot1, sizeof(m), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    memcpy(&m, hs, sizeof(m));
    const int n1 = m.n;
    if (n1 == 0) return PSLFE_OK;
    PSL_REQUIRE(prev_matched && matches12, PSLFE_E_INVALID, "%s: NULL prev_matched / matches12 for %d keypoints", who, n1);
    // inputs and outputs through the pinned staging buffer: prev [n1][2], matches12 [n1], nmatches, the two slot numbers
    const size_t bp = psl_align_up((size_t)n1 * 2 * sizeof(float), 256), bm = psl_align_up((size_t)n1 * sizeof(int), 256);
    hs = psl_host_stage(ctx, bp + bm + 256);
    PSL_REQUIRE(hs, PSLFE_E_HIP, "%s: no pinned staging memory (hipHostMalloc)", who);
    float* h_prev = reinterpret_cast<float*>(hs);
    int* h_m12 = reinterpret_cast<int*>(hs + bp);
    int* h_misc = reinterpret_cast<int*>(hs + bp + bm);   // [0] nmatches, [1] slot1, [2] slot2
    memcpy(h_prev, prev_matched, (size_t)n1 * 2 * sizeof(float));
    h_misc[1] = slot1; h_misc[2] = slot2;
    if (int rc = psl_scratch_begin(ctx)) return rc;
    hipError_t e = hipSuccess;
    float* d_prev = psl_scratch_up(ctx, (const float*)nullptr, (size_t)f1->cap * 2, st, &e);   // rows n1.. are never read
    if (e == hipSuccess) e = hipMemcpyAsync(d_prev, h_prev, (size_t)n1 * 2 * sizeof(float), hipMemcpyHostToDevice, st);
    int* d_m12 = psl_scratch_up(ctx, (const int*)nullptr, (size_t)f1->cap, st, &e);
    int* d_misc = psl_scratch_up(ctx, h_misc, 3, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    int rc = mono_search(f1, d_misc + 1, f2, d_misc + 2, 1, d_prev, f1->cap, window, nnratio, check_orientation, d_m12, d_misc, who);
    if (rc) { (void)hipStreamSynchronize(st); return rc; }
    PSL_HIP(hipMemcpyAsync(h_prev, d_prev, (size_t)n1 * 2 * sizeof(float), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(h_m12, d_m12, (size_t)n1 * sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(h_misc, d_misc, sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    memcpy(prev_matched, h_prev, (size_t)n1 * 2 * sizeof(float));
    memcpy(matches12, h_m12, (size_t)n1 * sizeof(int));
    *nmatches = h_misc[0];
    return PSLFE_OK;
}

}  // extern "C"
