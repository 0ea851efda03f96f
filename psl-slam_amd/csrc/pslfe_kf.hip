// libpslfe: the KeyFrame-rate matchers of LocalMapping / LoopClosing. Product code.
// Reference behaviour reproduced, from the point where the host has projected its map points / lines:
//   ORBmatcher::Fuse (both)                     src/ORBmatcher.cc:825-966, 968-1100
//   ORBmatcher::SearchBySim3                    src/ORBmatcher.cc:1102-1326
//   ORBmatcher::SearchForTriangulation          src/ORBmatcher.cc:657-823 (+ CheckDistEpipolarLine :140-157)
//   KeyFrame::GetFeaturesInArea / GetLinesInArea src/KeyFrame.cc:685-724, 857-891
//   LSDmatcher::Fuse                            add_src/LSDmatcher.cpp:847-984
//   MapPoint / MapLine::ComputeDistinctiveDescriptors  src/MapPoint.cc:242-304, add_src/MapLine.cpp:250-310
//
// None of these has the first-come-first-served coupling of the Tracking matchers (vbMatched2 of SearchForTriangulation
// is never written, src/ORBmatcher.cc:686), so every query is one wave: lanes take the candidates, a key
// (distance << 16 | visiting order) is min-reduced across the wave, and the reference's tie rule is the key's low half.
#include <limits.h>
#include <string.h>

#include "match_kernels.h"
#include "kf_project.h"
#include "kf_line_kernels.h"
#include "triangulate_kernels.h"

#define PSL_KF_LEVELS 16
#define PSL_DISTINCT_MAX 1024  // observations of one map point handled (36 KB of descriptors in LDS)

struct BestArgs {
    FrameStore S;
    int slot;
    const PslProjQuery* q;
    const uint8_t* qdesc;
    int nq, chi2;
    float inv_sigma2[PSL_KF_LEVELS];
    int* best_idx;
    int* best_dist;
};

// Fuse / SearchBySim3 candidate loop of one projected map point against slot `slot`, by one wave: row qi of the queries, descriptor
// row di; lane 0 writes best_idx[qi] / best_dist[qi].
__device__ __forceinline__ void psl_window_best_row(const BestArgs& A, int slot, int qi, int di, int lane) {
    const PslProjQuery q = A.q[qi];
    if (!(q.radius >= 0)) {
        if (lane == 0) { A.best_idx[qi] = -1; A.best_dist[qi] = INT_MAX; }
        return;
    }
    const FrameView V = psl_frame_view(A.S, slot);
    const uint32_t* QD = reinterpret_cast<const uint32_t*>(A.qdesc + (size_t)di * 32);
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) qd[k] = QD[k];
    const WindowCols W = psl_window_cols(V, q, nullptr);
    const int lvl = q.max_level;
    const float r = q.radius;
    uint32_t best = PSL_KEY_INF;
    for (int base = 0; base < W.T; base += 64) {
        const int p = psl_window_pos(W, base + lane);
        if (p < 0) continue;  // (shuffles are done: the rest is lane-local)
        const int i2 = V.gidx[p];
        if (i2 < 0 || i2 >= V.n) continue;
        const float2 xy = *reinterpret_cast<const float2*>(&V.kps[i2].x);
        const int octave = V.kps[i2].octave;
        bool ok = __builtin_fabsf(PSL_FSUB(xy.x, q.u)) < r && __builtin_fabsf(PSL_FSUB(xy.y, q.v)) < r;
        ok = ok && !(octave < lvl - 1 || octave > lvl);
        if (ok && A.chi2) {  // src/ORBmatcher.cc:907-934
            const float kr = V.uright[i2];
            const float ex = PSL_FSUB(q.u, xy.x), ey = PSL_FSUB(q.v, xy.y);
            float e2 = PSL_FADD(PSL_FMUL(ex, ex), PSL_FMUL(ey, ey));
            const float is2 = A.inv_sigma2[octave & (PSL_KF_LEVELS - 1)];
            if (kr >= 0) {
                const float er = PSL_FSUB(q.ur, kr);
                e2 = PSL_FADD(e2, PSL_FMUL(er, er));
                ok = !((double)PSL_FMUL(e2, is2) > 7.8);
            } else {
                ok = !((double)PSL_FMUL(e2, is2) > 5.99);
            }
        }
        if (!ok) continue;
        const int dist = psl_hamming256(qd, V.desc + (size_t)i2 * 8);
        best = min(best, ((uint32_t)dist << 16) | (uint32_t)p);
    }
    best = psl_wave_min_u32(best);
    if (lane == 0) {
        A.best_idx[qi] = best == PSL_KEY_INF ? -1 : V.gidx[best & 0xffffu];
        A.best_dist[qi] = best == PSL_KEY_INF ? INT_MAX : (int)(best >> 16);
    }
}

// one keyframe: one wave per projected map point
__global__ __launch_bounds__(256) void k_window_best(BestArgs A) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (qi >= A.nq) return;
    psl_window_best_row(A, A.slot, qi, qi, lane);
}

// K keyframes x M map points (pslfe_kf_fuse_keyframes): one wave per row k*M + i of pslfe_kf_project, searched in slot views[k].slot
// with the descriptor of map point i.  Keyframes on blockIdx.y: the waves of a workgroup read one keyframe's grid.
__global__ __launch_bounds__(256) void k_window_best_set(BestArgs A, const PslKfView* __restrict__ views) {
    const int i = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, k = blockIdx.y;
    if (i >= A.nq) return;   // nq = M
    psl_window_best_row(A, views[k].slot, k * A.nq + i, i, lane);
}

// SearchBySim3 agreement check (src/ORBmatcher.cc:1225-1232, 1296-1323)
__global__ __launch_bounds__(256) void k_sim3_agree(const int* __restrict__ b1, const int* __restrict__ d1, int n1, const int* __restrict__ b2,
                                                     const int* __restrict__ d2, int n2, int* __restrict__ match12, int* __restrict__ nfound) {
    const int i1 = blockIdx.x * 256 + threadIdx.x;
    bool found = false;
    if (i1 < n1) {
        const int idx2 = d1[i1] <= PSL_TH_HIGH ? b1[i1] : -1;
        int m = -1;
        if (idx2 >= 0 && idx2 < n2) {
            const int idx1 = d2[idx2] <= PSL_TH_HIGH ? b2[idx2] : -1;
            if (idx1 == i1) m = idx2;
        }
        match12[i1] = m;
        found = m >= 0;
    }
    const int c = __popcll(__ballot(found));
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(nfound, c);
}

struct TriArgs {
    FrameStore S;
    int slot;
    const int* fidx;
    int nfidx;
    const uint8_t* taken;
    const PslTriQuery* q;
    const uint8_t* qdesc;
    int nq;
    float F[9];
    float ex, ey;
    int only_stereo, check_ori;
    float sf[PSL_KF_LEVELS], sig2[PSL_KF_LEVELS];
    int* choice;
    int* match;
    int* nmatches;
};

// SearchForTriangulation candidate loop (src/ORBmatcher.cc:713-756) of one feature of KF1 by one wave: the chosen idx2 or -1, in every lane.
__device__ __forceinline__ int psl_tri_choice_row(const FrameView& V, const int* __restrict__ fidx, int nfidx, const uint8_t* __restrict__ taken,
                                                  const PslTriQuery& q, const uint32_t* __restrict__ QD, const float* F, float epx, float epy,
                                                  int only_stereo, const float* sf, const float* sig2, int lane) {
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) qd[k] = QD[k];
    // epipolar line in the second image l = x1' F12 = [a b c]
    const float a = PSL_FADD(PSL_FADD(PSL_FMUL(q.x, F[0]), PSL_FMUL(q.y, F[3])), F[6]);
    const float b = PSL_FADD(PSL_FADD(PSL_FMUL(q.x, F[1]), PSL_FMUL(q.y, F[4])), F[7]);
    const float c = PSL_FADD(PSL_FADD(PSL_FMUL(q.x, F[2]), PSL_FMUL(q.y, F[5])), F[8]);
    const float den = PSL_FADD(PSL_FMUL(a, a), PSL_FMUL(b, b));
    const int start = max(q.start, 0), len = min(q.len, nfidx - start);
    uint32_t best = PSL_KEY_INF;
    for (int j = lane; j < len; j += 64) {
        const int idx2 = fidx[start + j];
        if (idx2 < 0 || idx2 >= V.n) continue;
        if (taken[idx2]) continue;
        const bool stereo2 = V.uright[idx2] >= 0;
        if (only_stereo && !stereo2) continue;
        const int dist = psl_hamming256(qd, V.desc + (size_t)idx2 * 8);
        if (dist > PSL_TH_LOW) continue;
        const float2 xy = *reinterpret_cast<const float2*>(&V.kps[idx2].x);
        const int octave = V.kps[idx2].octave & (PSL_KF_LEVELS - 1);
        if (!q.stereo && !stereo2) {
            const float dx = PSL_FSUB(epx, xy.x), dy = PSL_FSUB(epy, xy.y);
            if (PSL_FADD(PSL_FMUL(dx, dx), PSL_FMUL(dy, dy)) < PSL_FMUL(100.0f, sf[octave])) continue;
        }
        const float num = PSL_FADD(PSL_FADD(PSL_FMUL(a, xy.x), PSL_FMUL(b, xy.y)), c);
        if (den == 0) continue;
        const float dsqr = PSL_FDIV(PSL_FMUL(num, num), den);
        if (!((double)dsqr < PSL_DMUL(3.84, (double)sig2[octave]))) continue;
        // `dist > bestDist -> continue`: among equal distances the LAST visited candidate wins
        best = min(best, ((uint32_t)dist << 16) | (uint32_t)(0xffff - j));
    }
    best = psl_wave_min_u32(best);
    return best == PSL_KEY_INF ? -1 : fidx[start + (0xffff - (int)(best & 0xffffu))];
}

// one neighbour: one wave per feature of KF1
__global__ __launch_bounds__(256) void k_triangulation(TriArgs A) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (qi >= A.nq) return;
    const FrameView V = psl_frame_view(A.S, A.slot);
    const int c2 = psl_tri_choice_row(V, A.fidx, A.nfidx, A.taken, A.q[qi], reinterpret_cast<const uint32_t*>(A.qdesc + (size_t)qi * 32), A.F, A.ex, A.ey,
                                      A.only_stereo, A.sf, A.sig2, lane);
    if (lane == 0) A.choice[qi] = c2;
}

// rotation histogram + ComputeThreeMaxima + outputs (src/ORBmatcher.cc:764-811)
__global__ __launch_bounds__(1024) void k_triangulation_finish(TriArgs A) {
    __shared__ int s_hist[PSL_HISTO];
    __shared__ int s_ind[3];
    __shared__ int s_nm;
    __shared__ uint8_t s_bin[PSL_QMAX];
    const int tid = threadIdx.x;
    const FrameView V = psl_frame_view(A.S, A.slot);
    if (tid < PSL_HISTO) s_hist[tid] = 0;
    if (tid == 0) { s_ind[0] = s_ind[1] = s_ind[2] = -1; s_nm = 0; }
    __syncthreads();
    if (A.check_ori) {
        for (int qi = tid; qi < A.nq; qi += 1024) {
            const int c2 = A.choice[qi];
            if (c2 < 0) continue;
            const int bin = psl_rot_bin(A.q[qi].angle, V.kps[c2].angle);
            s_bin[qi] = (uint8_t)bin;
            atomicAdd(&s_hist[bin], 1);
        }
        __syncthreads();
        if (tid == 0) psl_three_maxima(s_hist, s_ind);
        __syncthreads();
    }
    int local = 0;
    for (int qi = tid; qi < A.nq; qi += 1024) {
        const int c2 = A.choice[qi];
        bool good = c2 >= 0;
        if (good && A.check_ori) good = psl_rot_keep(s_bin[qi], s_ind);
        A.match[qi] = good ? c2 : -1;
        local += good;
    }
    local = psl_wave_sum(local);
    if ((tid & 63) == 0 && local) atomicAdd(&s_nm, local);
    __syncthreads();
    if (tid == 0) *A.nmatches = s_nm;
}

// ---- CreateNewMapPoints (src/LocalMapping.cc:305-519): the candidate loops of all neighbours, then one resident workgroup --------------
#define PSL_NP_THREADS 256
struct NewPtsArgs {
    FrameStore S;
    PslTriKeyFrame kf1;
    int N1, K, nqmax, only_stereo, check_ori;
    float sf[PSL_KF_LEVELS], sig2[PSL_KF_LEVELS];
    const PslTriNeighbour* nb;   // [K]
    const int* fidx_off;         // [K+1]
    const int* kp_off;           // [K+1]
    const int* nq;               // [K]
    const PslKeyPoint* keysun1;
    const float* keys1;
    const float* uright1;
    const float* depth1;
    const uint8_t* taken1;
    const int* fidx2;
    const uint8_t* taken2;
    const float* keys2;
    const float* depth2;
    const PslTriQuery* q;
    const int* idx1;
    const uint8_t* qdesc;
    int* choice;                 // [K][nqmax]
    int* match;
    int* status;
    float* x3d;
    int* nmatches;
    int* created_by;
    PslNewMapPoint* newp;
    int* nnew;
    PslMapPointGeom* geom;       // may be nullptr
    int* obs_off;                // the four observation arrays: all or none
    int* obs_kf;
    int* ref_kf;
    int* ref_level;
};

// The candidate loop does not read taken1: every (neighbour, query) at once, one wave each, neighbours on blockIdx.y.
__global__ __launch_bounds__(256) void k_new_points_choice(NewPtsArgs A) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63, k = blockIdx.y;
    if (qi >= min(A.nq[k], A.nqmax)) return;
    const size_t row = (size_t)k * A.nqmax + qi;
    const PslTriNeighbour* nb = A.nb + k;
    int c2 = -1;
    if (nb->active) {
        FrameView V = psl_frame_view(A.S, nb->slot);
        V.n = min(V.n, A.kp_off[k + 1] - A.kp_off[k]);   // a keypoint without a row in taken2 / keys2 / depth2 is no candidate
        float F[9];
#pragma unroll
        for (int i = 0; i < 9; ++i) F[i] = nb->F12[i];
        c2 = psl_tri_choice_row(V, A.fidx2 + A.fidx_off[k], A.fidx_off[k + 1] - A.fidx_off[k], A.taken2 + A.kp_off[k], A.q[row],
                                reinterpret_cast<const uint32_t*>(A.qdesc + row * 32), F, nb->ex, nb->ey, A.only_stereo, A.sf, A.sig2, lane);
    }
    if (lane == 0) A.choice[row] = c2;
}

// One workgroup walks the neighbours in order.  Per neighbour: the rotation histogram over the queries whose feature is still free
// (src/ORBmatcher.cc:699-703 comes before :764-775), the three maxima, the matched pairs in the order of vMatchedPairs (idx1 ascending),
// one thread per pair for the body (SVD workspaces interleaved in LDS), the created ones appended in that order, taken1 marked.
__global__ __launch_bounds__(PSL_NP_THREADS) void k_new_points_finish(NewPtsArgs A) {
    __shared__ float s_wf[PSL_TRI_WS_F * PSL_NP_THREADS];
    __shared__ double s_wd[PSL_TRI_WS_D * PSL_NP_THREADS];
    __shared__ int16_t s_qof[PSL_QMAX];     // feature of KF1 -> its matched query of this neighbour, -1: none
    __shared__ uint16_t s_list[PSL_QMAX];   // the matched queries, idx1 ascending; | 0x8000: created
    __shared__ uint8_t s_taken[PSL_QMAX];
    __shared__ int s_hist[PSL_HISTO];
    __shared__ int s_ind[3];
    __shared__ int s_w[4];
    __shared__ int s_nm;
    __shared__ PslTriCam s_c1, s_c2;
    const int tid = threadIdx.x, N1 = A.N1, nqmax = A.nqmax;
    for (int i = tid; i < N1; i += PSL_NP_THREADS) { s_taken[i] = A.taken1[i] != 0; A.created_by[i] = -1; }
    if (tid == 0) psl_tri_cam_setup(&A.kf1.Tcw, A.kf1.fx, A.kf1.fy, A.kf1.cx, A.kf1.cy, A.kf1.mb, &s_c1);
    int nnew = 0;   // the same in every thread
    for (int k = 0; k < A.K; ++k) {
        const PslTriNeighbour* nb = A.nb + k;
        const size_t base = (size_t)k * nqmax;
        const int nq = min(max(A.nq[k], 0), nqmax);
        const bool active = nb->active != 0;
        __syncthreads();   // the previous neighbour's s_taken, s_list, s_c2
        if (tid < PSL_HISTO) s_hist[tid] = 0;
        if (tid == 0) {
            s_ind[0] = s_ind[1] = s_ind[2] = -1; s_nm = 0;
            psl_tri_cam_setup(&nb->Tcw, nb->fx, nb->fy, nb->cx, nb->cy, nb->mb, &s_c2);
        }
        for (int i = tid; i < N1; i += PSL_NP_THREADS) s_qof[i] = -1;
        __syncthreads();
        const FrameView V = psl_frame_view(A.S, active ? nb->slot : 0);
        if (active && A.check_ori) {
            for (int q = tid; q < nq; q += PSL_NP_THREADS) {
                const int c2 = A.choice[base + q], i1 = A.idx1[base + q];
                if (c2 < 0 || i1 < 0 || i1 >= N1 || s_taken[i1]) continue;
                atomicAdd(&s_hist[psl_rot_bin(A.q[base + q].angle, V.kps[c2].angle)], 1);
            }
            __syncthreads();
            if (tid == 0) psl_three_maxima(s_hist, s_ind);
            __syncthreads();
        }
        int local = 0;
        for (int q = tid; q < nqmax; q += PSL_NP_THREADS) {
            int st = PSL_TRI_NO_MATCH, m = -1;
            if (q < nq) {
                const int i1 = A.idx1[base + q];
                const bool in = i1 >= 0 && i1 < N1;
                if (!active) st = PSL_TRI_INACTIVE;
                else if (in && s_taken[i1]) st = PSL_TRI_TAKEN;
                else if (in) {
                    const int c2 = A.choice[base + q];
                    bool good = c2 >= 0;
                    if (good && A.check_ori) good = psl_rot_keep(psl_rot_bin(A.q[base + q].angle, V.kps[c2].angle), s_ind);
                    if (good) { m = c2; s_qof[i1] = (int16_t)q; ++local; }
                }
            }
            A.match[base + q] = m; A.status[base + q] = st;   // a matched row's status follows
            A.x3d[3 * (base + q)] = 0.f; A.x3d[3 * (base + q) + 1] = 0.f; A.x3d[3 * (base + q) + 2] = 0.f;
        }
        local = psl_wave_sum(local);
        if ((tid & 63) == 0 && local) atomicAdd(&s_nm, local);
        __syncthreads();
        const int nm = s_nm;
        if (tid == 0) A.nmatches[k] = nm;
        if (nm == 0) continue;   // uniform
        // the matched queries in idx1 order
        const int per = (N1 + PSL_NP_THREADS - 1) / PSL_NP_THREADS, i0 = tid * per, i9 = min(i0 + per, N1);
        int cnt = 0, total;
        for (int i = i0; i < i9; ++i) cnt += s_qof[i] >= 0;
        int pos = psl_block_scan_256(cnt, s_w, &total);
        for (int i = i0; i < i9; ++i)
            if (s_qof[i] >= 0) s_list[pos++] = (uint16_t)s_qof[i];
        const int np = total;   // == nm when idx1 is distinct inside the neighbour, as the header asks; never more entries than s_list holds
        __syncthreads();
        // the body of :354-499, one pair per thread
        for (int r = tid; r < np; r += PSL_NP_THREADS) {
            const int q = s_list[r], i1 = A.idx1[base + q], i2 = A.match[base + q];
            const PslKeyPoint k1 = A.keysun1[i1], k2 = V.kps[i2];
            const size_t g2 = (size_t)A.kp_off[k] + i2;
            const PslTriObs o1 = {k1.x, k1.y, A.keys1[2 * i1], A.keys1[2 * i1 + 1], A.uright1[i1], A.depth1[i1], k1.octave};
            const PslTriObs o2 = {k2.x, k2.y, A.keys2[2 * g2], A.keys2[2 * g2 + 1], V.uright[i2], A.depth2[g2], k2.octave};
            float p[3];
            const int st = psl_tri_point_row<PSL_NP_THREADS>(&s_c1, &s_c2, A.kf1.mbf, &o1, &o2, A.sf, A.sig2, A.kf1.ratio_factor, s_wf + tid, s_wd + tid, p);
            A.status[base + q] = st;
            A.x3d[3 * (base + q)] = p[0]; A.x3d[3 * (base + q) + 1] = p[1]; A.x3d[3 * (base + q) + 2] = p[2];
            if (st == PSL_TRI_CREATED) s_list[r] = (uint16_t)(q | 0x8000);
        }
        __syncthreads();
        // the created ones, appended in the same order
        const int rper = (np + PSL_NP_THREADS - 1) / PSL_NP_THREADS, r0 = tid * rper, r9 = min(r0 + rper, np);
        cnt = 0;
        for (int r = r0; r < r9; ++r) cnt += s_list[r] >> 15;
        pos = nnew + psl_block_scan_256(cnt, s_w, &total);
        for (int r = r0; r < r9; ++r) {
            if (!(s_list[r] >> 15)) continue;
            const int q = s_list[r] & 0x7fff, i1 = A.idx1[base + q], i2 = A.match[base + q];
            const float x = A.x3d[3 * (base + q)], y = A.x3d[3 * (base + q) + 1], z = A.x3d[3 * (base + q) + 2];
            const PslNewMapPoint np = {x, y, z, k, i1, i2};
            A.newp[pos] = np;
            if (A.geom) { const PslMapPointGeom g = {x, y, z, 0.f, 0.f, 0.f, 0.f, 0.f}; A.geom[pos] = g; }
            if (A.obs_kf) {
                A.obs_kf[2 * pos] = nb->kf_first ? nb->kf : A.kf1.kf;
                A.obs_kf[2 * pos + 1] = nb->kf_first ? A.kf1.kf : nb->kf;
                A.ref_kf[pos] = A.kf1.kf;
                A.ref_level[pos] = A.keysun1[i1].octave;
            }
            s_taken[i1] = 1;
            A.created_by[i1] = k;
            ++pos;
        }
        nnew += total;
    }
    if (tid == 0) *A.nnew = nnew;
    if (A.obs_off)
        for (int r = tid; r <= N1; r += PSL_NP_THREADS) A.obs_off[r] = 2 * min(r, nnew);
}

// LSDmatcher::Fuse search: KeyFrame::GetLinesInArea is a linear scan of the keyframe's keylines; one wave per map line.
__global__ __launch_bounds__(256) void k_line_fuse_best(const PslKeyLine* __restrict__ kls, int n, const uint8_t* __restrict__ desc, int ndesc,
                                                         const PslLineFuseQuery* __restrict__ Q, const uint8_t* __restrict__ qdesc, int nq,
                                                         int* __restrict__ best_idx, int* __restrict__ best_dist) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (qi >= nq) return;
    const LineFuseGlobal S = {kls, reinterpret_cast<const uint32_t*>(desc)};
    psl_line_fuse_row(S, n, ndesc, Q[qi], qdesc + (size_t)qi * 32, lane, best_idx + qi, best_dist + qi);
}

// ComputeDistinctiveDescriptors: one wave per map point.  Row i of the distance matrix lives in the lanes' registers
// (lane l holds columns l, l + 64, ...); its median sorted[k], k = floor(0.5 (N - 1)), is the smallest value v with
// #{d <= v} >= k + 1, found by bisection on v in [0, 256] with ballot-free popcount sums.
__global__ __launch_bounds__(64) void k_distinctive(const uint8_t* __restrict__ desc, const int* __restrict__ offsets, int npts, int* __restrict__ best) {
    __shared__ uint32_t s_d[PSL_DISTINCT_MAX * 9];  // rows padded to 9 words: conflict-free column reads
    const int p = blockIdx.x, lane = threadIdx.x;
    if (p >= npts) return;
    const int o0 = offsets[p];
    int N = offsets[p + 1] - o0;
    if (N <= 0) {
        if (lane == 0) best[p] = -1;
        return;
    }
    N = min(N, PSL_DISTINCT_MAX);
    const uint32_t* D = reinterpret_cast<const uint32_t*>(desc) + (size_t)o0 * 8;
    for (int i = lane; i < N * 8; i += 64) s_d[(i >> 3) * 9 + (i & 7)] = D[i];
    __syncthreads();
    const int k = (int)(0.5 * (double)(N - 1));
    constexpr int PER = PSL_DISTINCT_MAX / 64;
    uint32_t bestKey = PSL_KEY_INF;  // median << 16 | row
    for (int i = 0; i < N; ++i) {
        uint32_t qd[8];
#pragma unroll
        for (int w = 0; w < 8; ++w) qd[w] = s_d[i * 9 + w];
        int d[PER];
#pragma unroll
        for (int t = 0; t < PER; ++t) {
            const int j = lane + 64 * t;
            d[t] = 0x7fff;
            if (t * 64 < N && j < N) {
                int s = 0;
#pragma unroll
                for (int w = 0; w < 8; ++w) s += __popc(qd[w] ^ s_d[j * 9 + w]);
                d[t] = s;
            }
        }
        int lo = 0, hi = 256;  // smallest v with count(d <= v) >= k + 1
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            int cnt = 0;
#pragma unroll
            for (int t = 0; t < PER; ++t)
                if (t * 64 < N) cnt += d[t] <= mid;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);  // not psl_wave_sum: the call changes this kernel's registers (77 -> 62 VGPRs, +65 instructions)
            if (cnt >= k + 1) hi = mid; else lo = mid + 1;
        }
        bestKey = min(bestKey, ((uint32_t)lo << 16) | (uint32_t)i);
    }
    if (lane == 0) best[p] = (int)(bestKey & 0xffffu);
}

// ---------------------------------------------------------------------------------------------
namespace {
int check_slot(pslfe_frame* f, int slot, const char* who) {
    PSL_REQUIRE(f, PSLFE_E_INVALID, "%s: NULL frame", who);
    PSL_REQUIRE(slot >= 0 && slot < f->max_frames && f->slot_set[slot], PSLFE_E_STATE, "%s: slot %d not set", who, slot);
    return PSLFE_OK;
}

int launch_window_best(pslfe_kf* k, pslfe_frame* f, int slot, const PslProjQuery* d_q, const uint8_t* d_qdesc, int nq, int chi2,
                       const float* inv_sigma2, int nlevels, int* d_idx, int* d_dist) {
    BestArgs A;
    A.S = f->S; A.slot = slot; A.q = d_q; A.qdesc = d_qdesc; A.nq = nq; A.chi2 = chi2;
    for (int i = 0; i < PSL_KF_LEVELS; ++i) A.inv_sigma2[i] = (inv_sigma2 && i < nlevels) ? inv_sigma2[i] : 0.f;
    A.best_idx = d_idx; A.best_dist = d_dist;
    k_window_best<<<(nq + 3) / 4, 256, 0, k->ctx->stream>>>(A);
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

// a slot a PslKfView names: PSLFE_E_INVALID outside the store, PSLFE_E_STATE when it was never set
int check_view_slot(pslfe_frame* f, int slot, const char* who) {
    PSL_REQUIRE(slot >= 0 && slot < f->max_frames, PSLFE_E_INVALID, "%s: slot %d outside the store (0..%d)", who, slot, f->max_frames - 1);
    PSL_REQUIRE(f->slot_set[slot], PSLFE_E_STATE, "%s: slot %d not set", who, slot);
    return PSLFE_OK;
}

// both directions and the agreement check of SearchBySim3 on device rows; d_m [n1], d_nf [1]
int launch_sim3(pslfe_kf* k, pslfe_frame* f1, int slot1, pslfe_frame* f2, int slot2, const PslProjQuery* d_q1, const uint8_t* d_qd1, int n1,
                const PslProjQuery* d_q2, const uint8_t* d_qd2, int n2, int* d_m, int* d_nf) {
    hipStream_t st = k->ctx->stream;
    const size_t m1 = (size_t)n1, m2 = (size_t)(n2 > 0 ? n2 : 1);
    hipError_t e = hipSuccess;
    int* d_b1 = psl_scratch_up(k->ctx, (const int*)nullptr, m1, st, &e);
    int* d_d1 = psl_scratch_up(k->ctx, (const int*)nullptr, m1, st, &e);
    int* d_b2 = psl_scratch_up(k->ctx, (const int*)nullptr, m2, st, &e);
    int* d_d2 = psl_scratch_up(k->ctx, (const int*)nullptr, m2, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "SearchBySim3: %s", hipGetErrorString(e));
    PSL_HIP(hipMemsetAsync(d_nf, 0, 4, st));
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.sim3");
        if (int rc = launch_window_best(k, f2, slot2, d_q1, d_qd1, n1, 0, nullptr, 0, d_b1, d_d1)) return rc;
        if (n2 > 0)
            if (int rc = launch_window_best(k, f1, slot1, d_q2, d_qd2, n2, 0, nullptr, 0, d_b2, d_d2)) return rc;
        k_sim3_agree<<<(n1 + 255) / 256, 256, 0, st>>>(d_b1, d_d1, n1, d_b2, d_d2, n2, d_m, d_nf);
        PSL_STAGE_END(k->ctx, "kf.sim3");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}
}  // namespace

extern "C" {

int pslfe_kf_create(pslfe_ctx* ctx, pslfe_kf** out) {
    PSL_REQUIRE(ctx && out, PSLFE_E_INVALID, "pslfe_kf_create: NULL argument");
    pslfe_kf* k = new pslfe_kf();
    k->ctx = ctx;
    *out = k;
    return PSLFE_OK;
}

void pslfe_kf_destroy(pslfe_kf* k) {
    delete k;
}

int pslfe_kf_window_best(pslfe_kf* k, pslfe_frame* f, int slot, const PslProjQuery* queries, const uint8_t* qdesc, int nq, int chi2,
                         const float* inv_level_sigma2, int nlevels, int32_t* best_idx, int32_t* best_dist) {
    PSL_REQUIRE(k && (nq == 0 || (queries && qdesc && best_idx && best_dist)), PSLFE_E_INVALID, "pslfe_kf_window_best: NULL argument");
    PSL_REQUIRE(nq >= 0, PSLFE_E_INVALID, "pslfe_kf_window_best: nq = %d", nq);
    PSL_REQUIRE(!chi2 || (inv_level_sigma2 && nlevels > 0 && nlevels <= PSL_KF_LEVELS), PSLFE_E_INVALID,
                "pslfe_kf_window_best: chi2 gates need mvInvLevelSigma2 with 1..%d levels", PSL_KF_LEVELS);
    if (int rc = check_slot(f, slot, "pslfe_kf_window_best")) return rc;
    if (nq == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    PslProjQuery* d_q = psl_scratch_up(k->ctx, queries, nq, st, &e);
    uint8_t* d_qd = psl_scratch_up(k->ctx, qdesc, (size_t)nq * 32, st, &e);
    int* d_i = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    int* d_d = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "pslfe_kf_window_best: %s", hipGetErrorString(e));
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.window_best");
        if (int rc = launch_window_best(k, f, slot, d_q, d_qd, nq, chi2, inv_level_sigma2, nlevels, d_i, d_d)) return rc;
        PSL_STAGE_END(k->ctx, "kf.window_best");
    }
    PSL_HIP(hipMemcpyAsync(best_idx, d_i, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(best_dist, d_d, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_search_by_sim3(pslfe_kf* k, pslfe_frame* f1, int slot1, pslfe_frame* f2, int slot2, const PslProjQuery* q12,
                            const uint8_t* qdesc1, int n1, const PslProjQuery* q21, const uint8_t* qdesc2, int n2, int32_t* match12,
                            int* nfound) {
    PSL_REQUIRE(k && nfound && (n1 == 0 || (q12 && qdesc1 && match12)) && (n2 == 0 || (q21 && qdesc2)), PSLFE_E_INVALID,
                "pslfe_kf_search_by_sim3: NULL argument");
    PSL_REQUIRE(n1 >= 0 && n2 >= 0, PSLFE_E_INVALID, "pslfe_kf_search_by_sim3: negative count");
    if (int rc = check_slot(f1, slot1, "pslfe_kf_search_by_sim3")) return rc;
    if (int rc = check_slot(f2, slot2, "pslfe_kf_search_by_sim3")) return rc;
    *nfound = 0;
    if (n1 == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    const size_t m1 = (size_t)n1, m2 = (size_t)(n2 > 0 ? n2 : 1);
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    PslProjQuery* d_q1 = psl_scratch_up(k->ctx, q12, m1, st, &e);
    uint8_t* d_qd1 = psl_scratch_up(k->ctx, qdesc1, m1 * 32, st, &e);
    PslProjQuery* d_q2 = psl_scratch_up(k->ctx, n2 > 0 ? q21 : nullptr, m2, st, &e);
    uint8_t* d_qd2 = psl_scratch_up(k->ctx, n2 > 0 ? qdesc2 : nullptr, m2 * 32, st, &e);
    int* d_m = psl_scratch_up(k->ctx, (const int*)nullptr, m1, st, &e);
    int* d_nf = psl_scratch_up(k->ctx, (const int*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "pslfe_kf_search_by_sim3: %s", hipGetErrorString(e));
    if (int rc = launch_sim3(k, f1, slot1, f2, slot2, d_q1, d_qd1, n1, d_q2, d_qd2, n2, d_m, d_nf)) return rc;
    PSL_HIP(hipMemcpyAsync(match12, d_m, m1 * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nfound, d_nf, 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_fuse_keyframes(pslfe_kf* k, pslfe_frame* f, int mode, const PslKfView* views, int K, const PslMapPointGeom* mp,
                            const uint8_t* mpdesc, const uint8_t* skip, int M, const PslCamera* cam, float min_x, float min_y, float max_x,
                            float max_y, const float* scale_factors, const float* inv_level_sigma2, int nlevels, float log_scale_factor,
                            float th, int32_t* best_idx, int32_t* best_dist, PslProjQuery* queries) {
    static const char* who = "pslfe_kf_fuse_keyframes";
    PSL_REQUIRE(k && f, PSLFE_E_INVALID, "%s: NULL handle", who);
    PSL_REQUIRE(K >= 0 && M >= 0 && (double)K * (double)M <= (double)INT_MAX && K <= 65535, PSLFE_E_INVALID, "%s: K = %d, M = %d", who, K, M);
    PSL_REQUIRE(mode == PSLFE_KF_PROJ_FUSE || mode == PSLFE_KF_PROJ_SCW, PSLFE_E_INVALID, "%s: mode %d (0: Fuse(pKF, ...), 1: Fuse(pKF, Scw, ...))",
                who, mode);
    const int chi2 = mode == PSLFE_KF_PROJ_FUSE;
    PSL_REQUIRE(!chi2 || inv_level_sigma2, PSLFE_E_INVALID, "%s: the chi2 gates of mode 0 need mvInvLevelSigma2", who);
    ProjParams P;
    if (int rc = psl_proj_params(&P, mode, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, log_scale_factor, th, who)) return rc;
    if (K == 0 || M == 0) return PSLFE_OK;
    PSL_REQUIRE(views && mp && mpdesc && best_idx && best_dist, PSLFE_E_INVALID, "%s: NULL argument", who);
    for (int i = 0; i < K; ++i)
        if (int rc = check_view_slot(f, views[i].slot, who)) return rc;
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    const size_t rows = (size_t)K * M;
    KfProjBuffers B;
    if (int rc = psl_kf_project_upload(k->ctx, P, views, K, mp, skip, M, false, &B, who)) return rc;
    hipError_t e = hipSuccess;
    BestArgs A;
    A.S = f->S; A.slot = 0; A.q = B.q; A.nq = M; A.chi2 = chi2;
    A.qdesc = psl_scratch_up(k->ctx, mpdesc, (size_t)M * 32, st, &e);
    A.best_idx = psl_scratch_up(k->ctx, (const int*)nullptr, rows, st, &e);
    A.best_dist = psl_scratch_up(k->ctx, (const int*)nullptr, rows, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    for (int i = 0; i < PSL_KF_LEVELS; ++i) A.inv_sigma2[i] = (chi2 && i < nlevels) ? inv_level_sigma2[i] : 0.f;
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.window_best_set");
        k_window_best_set<<<dim3((M + 3) / 4, K), 256, 0, st>>>(A, B.views);
        PSL_STAGE_END(k->ctx, "kf.window_best_set");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(best_idx, A.best_idx, rows * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(best_dist, A.best_dist, rows * 4, hipMemcpyDeviceToHost, st));
    if (queries) PSL_HIP(hipMemcpyAsync(queries, B.q, rows * sizeof(PslProjQuery), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_search_by_sim3_poses(pslfe_kf* k, pslfe_frame* f1, pslfe_frame* f2, const PslKfView* view12, const PslMapPointGeom* mp1,
                                  const uint8_t* desc1, const uint8_t* skip1, int n1, const PslKfView* view21, const PslMapPointGeom* mp2,
                                  const uint8_t* desc2, const uint8_t* skip2, int n2, const PslCamera* cam, float min_x, float min_y,
                                  float max_x, float max_y, const float* scale_factors, int nlevels, float log_scale_factor, float th,
                                  int32_t* match12, int* nfound, PslProjQuery* q12, PslProjQuery* q21) {
    static const char* who = "pslfe_kf_search_by_sim3_poses";
    PSL_REQUIRE(k && f1 && f2, PSLFE_E_INVALID, "%s: NULL handle", who);
    PSL_REQUIRE(nfound && view12 && view21, PSLFE_E_INVALID, "%s: NULL view or output", who);
    PSL_REQUIRE(n1 >= 0 && n2 >= 0, PSLFE_E_INVALID, "%s: negative count", who);
    PSL_REQUIRE((n1 == 0 || (mp1 && desc1 && match12)) && (n2 == 0 || (mp2 && desc2)), PSLFE_E_INVALID, "%s: NULL argument", who);
    ProjParams P;
    if (int rc = psl_proj_params(&P, PSLFE_KF_PROJ_SIM3, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, log_scale_factor, th, who))
        return rc;
    if (int rc = check_view_slot(f2, view12->slot, who)) return rc;   // map points of KF1 are searched in KF2's image
    if (int rc = check_view_slot(f1, view21->slot, who)) return rc;
    *nfound = 0;
    if (n1 == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    KfProjBuffers B1, B2;
    B2.q = nullptr;
    if (int rc = psl_kf_project_upload(k->ctx, P, view12, 1, mp1, skip1, n1, false, &B1, who)) return rc;
    if (n2 > 0)
        if (int rc = psl_kf_project_upload(k->ctx, P, view21, 1, mp2, skip2, n2, false, &B2, who)) return rc;
    const size_t m1 = (size_t)n1, m2 = (size_t)(n2 > 0 ? n2 : 1);
    hipError_t e = hipSuccess;
    uint8_t* d_qd1 = psl_scratch_up(k->ctx, desc1, m1 * 32, st, &e);
    uint8_t* d_qd2 = psl_scratch_up(k->ctx, n2 > 0 ? desc2 : nullptr, m2 * 32, st, &e);
    int* d_m = psl_scratch_up(k->ctx, (const int*)nullptr, m1, st, &e);
    int* d_nf = psl_scratch_up(k->ctx, (const int*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    if (int rc = launch_sim3(k, f1, view21->slot, f2, view12->slot, B1.q, d_qd1, n1, B2.q, d_qd2, n2, d_m, d_nf)) return rc;
    PSL_HIP(hipMemcpyAsync(match12, d_m, m1 * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nfound, d_nf, 4, hipMemcpyDeviceToHost, st));
    if (q12) PSL_HIP(hipMemcpyAsync(q12, B1.q, m1 * sizeof(PslProjQuery), hipMemcpyDeviceToHost, st));
    if (q21 && n2 > 0) PSL_HIP(hipMemcpyAsync(q21, B2.q, (size_t)n2 * sizeof(PslProjQuery), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_search_for_triangulation(pslfe_kf* k, pslfe_frame* f2, int slot2, const int32_t* fidx2, int nfidx2, const uint8_t* taken2,
                                      const PslTriQuery* queries, const uint8_t* qdesc, int nq, const float* F12, float ex, float ey,
                                      int only_stereo, int check_orientation, const float* scale_factors, const float* level_sigma2,
                                      int nlevels, int32_t* match, int* nmatches) {
    PSL_REQUIRE(k && nmatches && F12 && scale_factors && level_sigma2 && (nq == 0 || (queries && qdesc && match)) &&
                    (nfidx2 == 0 || (fidx2 && taken2)),
                PSLFE_E_INVALID, "pslfe_kf_search_for_triangulation: NULL argument");
    PSL_REQUIRE(nq >= 0 && nq <= PSL_QMAX, PSLFE_E_INVALID, "pslfe_kf_search_for_triangulation: %d queries (max %d)", nq, PSL_QMAX);
    PSL_REQUIRE(nlevels > 0 && nlevels <= PSL_KF_LEVELS, PSLFE_E_INVALID, "pslfe_kf_search_for_triangulation: %d levels (max %d)", nlevels,
                PSL_KF_LEVELS);
    PSL_REQUIRE(nfidx2 >= 0 && nfidx2 <= 0xffff, PSLFE_E_CAPACITY, "pslfe_kf_search_for_triangulation: %d feature-vector entries", nfidx2);
    if (int rc = check_slot(f2, slot2, "pslfe_kf_search_for_triangulation")) return rc;
    *nmatches = 0;
    if (nq == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    FrameMeta m;
    PSL_HIP(hipMemcpyAsync(&m, f2->S.meta + slot2, sizeof(m), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    const size_t nf = (size_t)(nfidx2 > 0 ? nfidx2 : 1), nk = (size_t)(m.n > 0 ? m.n : 1);
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    TriArgs A;
    PslTriQuery* d_q = psl_scratch_up(k->ctx, queries, nq, st, &e);
    uint8_t* d_qd = psl_scratch_up(k->ctx, qdesc, (size_t)nq * 32, st, &e);
    int* d_fidx = psl_scratch_up(k->ctx, nfidx2 > 0 ? fidx2 : nullptr, nf, st, &e);
    uint8_t* d_taken = psl_scratch_up(k->ctx, (const uint8_t*)nullptr, nk, st, &e);
    A.choice = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    A.match = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    A.nmatches = psl_scratch_up(k->ctx, (const int*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "pslfe_kf_search_for_triangulation: %s", hipGetErrorString(e));
    if (m.n > 0 && taken2) PSL_HIP(hipMemcpyAsync(d_taken, taken2, (size_t)m.n, hipMemcpyHostToDevice, st));
    else PSL_HIP(hipMemsetAsync(d_taken, 0, nk, st));
    A.S = f2->S; A.slot = slot2; A.fidx = d_fidx; A.nfidx = nfidx2; A.taken = d_taken; A.q = d_q; A.qdesc = d_qd; A.nq = nq;
    memcpy(A.F, F12, sizeof(A.F));
    A.ex = ex; A.ey = ey; A.only_stereo = only_stereo; A.check_ori = check_orientation;
    for (int i = 0; i < PSL_KF_LEVELS; ++i) { A.sf[i] = i < nlevels ? scale_factors[i] : 0.f; A.sig2[i] = i < nlevels ? level_sigma2[i] : 0.f; }
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.triangulation");
        k_triangulation<<<(nq + 3) / 4, 256, 0, st>>>(A);
        k_triangulation_finish<<<1, 1024, 0, st>>>(A);
        PSL_STAGE_END(k->ctx, "kf.triangulation");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(match, A.match, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nmatches, A.nmatches, 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

// ---- CreateNewMapPoints -----------------------------------------------------------------------------------------------------------------
namespace {
// the checks both forms share, in the header's order; *done = 1: K == 0
int new_points_check(const char* who, pslfe_kf* k, pslfe_frame* f2, const PslTriKeyFrame* kf1, int N1, const PslTriNeighbour* nb, int K,
                     const int32_t* fidx_off, const int32_t* kp_off, const int32_t* nq, int nqmax, const float* scale_factors,
                     const float* level_sigma2, int nlevels, bool arrays, int* done) {
    *done = 0;
    PSL_REQUIRE(N1 >= 0 && N1 <= PSL_QMAX && nqmax >= 0 && nqmax <= PSL_QMAX && K >= 0 && K <= PSLFE_TRI_MAX_NEIGHBOURS, PSLFE_E_INVALID,
                "%s: N1 = %d, nqmax = %d (max %d), K = %d (max %d)", who, N1, nqmax, PSL_QMAX, K, PSLFE_TRI_MAX_NEIGHBOURS);
    if (K == 0) { *done = 1; return PSLFE_OK; }
    PSL_REQUIRE(k && f2 && kf1 && nb && fidx_off && kp_off && nq && scale_factors && level_sigma2 && arrays, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(nlevels > 0 && nlevels <= PSL_KF_LEVELS, PSLFE_E_INVALID, "%s: %d levels (max %d)", who, nlevels, PSL_KF_LEVELS);
    PSL_REQUIRE(fidx_off[0] == 0 && kp_off[0] == 0, PSLFE_E_INVALID, "%s: offsets must start at 0", who);
    for (int i = 0; i < K; ++i) {
        PSL_REQUIRE(fidx_off[i + 1] >= fidx_off[i] && kp_off[i + 1] >= kp_off[i], PSLFE_E_INVALID, "%s: offsets of neighbour %d descend", who, i);
        PSL_REQUIRE(nq[i] >= 0 && nq[i] <= nqmax, PSLFE_E_INVALID, "%s: nq[%d] = %d (nqmax %d)", who, i, nq[i], nqmax);
        PSL_REQUIRE(fidx_off[i + 1] - fidx_off[i] <= 0xffff, PSLFE_E_CAPACITY, "%s: neighbour %d has %d feature-vector entries", who, i,
                    fidx_off[i + 1] - fidx_off[i]);
    }
    for (int i = 0; i < K; ++i)   // an inactive neighbour is never searched: its slot is not looked at
        if (nb[i].active)
            if (int rc = check_view_slot(f2, nb[i].slot, who)) return rc;
    return PSLFE_OK;
}

// A: every device pointer set; uploads the per-neighbour host arrays and queues both kernels
int new_points_launch(const char* who, pslfe_kf* k, pslfe_frame* f2, NewPtsArgs& A, const PslTriKeyFrame* kf1, int N1, const PslTriNeighbour* nb, int K,
                      const int32_t* fidx_off, const int32_t* kp_off, const int32_t* nq, int nqmax, int only_stereo, int check_orientation,
                      const float* scale_factors, const float* level_sigma2, int nlevels) {
    hipStream_t st = k->ctx->stream;
    hipError_t e = hipSuccess;
    A.S = f2->S; A.kf1 = *kf1; A.N1 = N1; A.K = K; A.nqmax = nqmax; A.only_stereo = only_stereo; A.check_ori = check_orientation;
    for (int i = 0; i < PSL_KF_LEVELS; ++i) { A.sf[i] = i < nlevels ? scale_factors[i] : 0.f; A.sig2[i] = i < nlevels ? level_sigma2[i] : 0.f; }
    A.nb = psl_scratch_up(k->ctx, nb, K, st, &e);
    A.fidx_off = psl_scratch_up(k->ctx, fidx_off, (size_t)K + 1, st, &e);
    A.kp_off = psl_scratch_up(k->ctx, kp_off, (size_t)K + 1, st, &e);
    A.nq = psl_scratch_up(k->ctx, nq, K, st, &e);
    A.choice = psl_scratch_up(k->ctx, (const int*)nullptr, (size_t)K * (nqmax ? nqmax : 1), st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.new_points");
        if (nqmax > 0) k_new_points_choice<<<dim3((nqmax + 3) / 4, K), 256, 0, st>>>(A);
        k_new_points_finish<<<1, PSL_NP_THREADS, 0, st>>>(A);
        PSL_STAGE_END(k->ctx, "kf.new_points");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}
}  // namespace

int pslfe_kf_create_new_map_points_device(pslfe_kf* k, pslfe_frame* f2, const PslTriKeyFrame* kf1, int N1, const PslKeyPoint* d_keysun1,
                                          const float* d_keys1, const float* d_uright1, const float* d_depth1, const uint8_t* d_taken1,
                                          const PslTriNeighbour* nb, int K, const int32_t* d_fidx2, const int32_t* fidx_off, const uint8_t* d_taken2,
                                          const float* d_keys2, const float* d_depth2, const int32_t* kp_off, const PslTriQuery* d_queries,
                                          const int32_t* d_idx1, const uint8_t* d_qdesc, const int32_t* nq, int nqmax, int only_stereo,
                                          int check_orientation, const float* scale_factors, const float* level_sigma2, int nlevels, int32_t* d_match,
                                          int32_t* d_status, float* d_x3d, int32_t* d_nmatches, int32_t* d_created_by, PslNewMapPoint* d_newp,
                                          int32_t* d_nnew, PslMapPointGeom* d_geom, int32_t* d_obs_off, int32_t* d_obs_kf, int32_t* d_ref_kf,
                                          int32_t* d_ref_level) {
    static const char* who = "pslfe_kf_create_new_map_points_device";
    int done;
    const bool arrays = d_keysun1 && d_keys1 && d_uright1 && d_depth1 && d_taken1 && d_fidx2 && d_taken2 && d_keys2 && d_depth2 && d_queries && d_idx1 &&
                        d_qdesc && d_match && d_status && d_x3d && d_nmatches && d_created_by && d_newp && d_nnew && d_geom && d_obs_off && d_obs_kf &&
                        d_ref_kf && d_ref_level;
    if (int rc = new_points_check(who, k, f2, kf1, N1, nb, K, fidx_off, kp_off, nq, nqmax, scale_factors, level_sigma2, nlevels, arrays, &done)) return rc;
    if (done) return PSLFE_OK;
    PSL_HIP(hipSetDevice(k->ctx->device));
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    NewPtsArgs A;
    A.keysun1 = d_keysun1; A.keys1 = d_keys1; A.uright1 = d_uright1; A.depth1 = d_depth1; A.taken1 = d_taken1; A.fidx2 = d_fidx2; A.taken2 = d_taken2;
    A.keys2 = d_keys2; A.depth2 = d_depth2; A.q = d_queries; A.idx1 = d_idx1; A.qdesc = d_qdesc; A.match = d_match; A.status = d_status; A.x3d = d_x3d;
    A.nmatches = d_nmatches; A.created_by = d_created_by; A.newp = d_newp; A.nnew = d_nnew; A.geom = d_geom; A.obs_off = d_obs_off; A.obs_kf = d_obs_kf;
    A.ref_kf = d_ref_kf; A.ref_level = d_ref_level;
    return new_points_launch(who, k, f2, A, kf1, N1, nb, K, fidx_off, kp_off, nq, nqmax, only_stereo, check_orientation, scale_factors, level_sigma2, nlevels);
}

int pslfe_kf_create_new_map_points(pslfe_kf* k, pslfe_frame* f2, const PslTriKeyFrame* kf1, int N1, const PslKeyPoint* keysun1, const float* keys1,
                                   const float* uright1, const float* depth1, const uint8_t* taken1, const PslTriNeighbour* nb, int K,
                                   const int32_t* fidx2, const int32_t* fidx_off, const uint8_t* taken2, const float* keys2, const float* depth2,
                                   const int32_t* kp_off, const PslTriQuery* queries, const int32_t* idx1, const uint8_t* qdesc, const int32_t* nq,
                                   int nqmax, int only_stereo, int check_orientation, const float* scale_factors, const float* level_sigma2,
                                   int nlevels, int32_t* match, int32_t* status, float* x3d, int32_t* nmatches, int32_t* created_by,
                                   PslNewMapPoint* newp, int32_t* nnew, PslMapPointGeom* geom) {
    static const char* who = "pslfe_kf_create_new_map_points";
    int done;
    const bool arrays = nmatches && nnew && (N1 == 0 || (keysun1 && keys1 && uright1 && depth1 && taken1 && created_by && newp)) &&
                        (nqmax == 0 || (queries && idx1 && qdesc && match && status));
    if (int rc = new_points_check(who, k, f2, kf1, N1, nb, K, fidx_off, kp_off, nq, nqmax, scale_factors, level_sigma2, nlevels, arrays, &done)) return rc;
    if (done) return PSLFE_OK;
    PSL_REQUIRE((fidx_off[K] == 0 || fidx2) && (kp_off[K] == 0 || (taken2 && keys2 && depth2)), PSLFE_E_INVALID, "%s: NULL neighbour arrays", who);
    {
        std::vector<int> seen((size_t)N1 + 1, -1);
        for (int i = 0; i < K; ++i)
            for (int q = 0; q < nq[i]; ++q) {
                const int i1 = idx1[(size_t)i * nqmax + q];
                PSL_REQUIRE(i1 >= 0 && i1 < N1, PSLFE_E_INVALID, "%s: idx1 %d of neighbour %d, query %d outside [0, %d)", who, i1, i, q, N1);
                PSL_REQUIRE(seen[i1] != i, PSLFE_E_INVALID, "%s: feature %d twice in the queries of neighbour %d", who, i1, i);
                seen[i1] = i;
            }
    }
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    const size_t n1 = N1 ? N1 : 1, rows = (size_t)K * (nqmax ? nqmax : 1), nf = fidx_off[K] ? fidx_off[K] : 1, nk = kp_off[K] ? kp_off[K] : 1;
    NewPtsArgs A;
    A.keysun1 = psl_scratch_up(k->ctx, N1 ? keysun1 : nullptr, n1, st, &e);
    A.keys1 = psl_scratch_up(k->ctx, N1 ? keys1 : nullptr, 2 * n1, st, &e);
    A.uright1 = psl_scratch_up(k->ctx, N1 ? uright1 : nullptr, n1, st, &e);
    A.depth1 = psl_scratch_up(k->ctx, N1 ? depth1 : nullptr, n1, st, &e);
    A.taken1 = psl_scratch_up(k->ctx, N1 ? taken1 : nullptr, n1, st, &e);
    A.fidx2 = psl_scratch_up(k->ctx, fidx_off[K] ? fidx2 : nullptr, nf, st, &e);
    A.taken2 = psl_scratch_up(k->ctx, kp_off[K] ? taken2 : nullptr, nk, st, &e);
    A.keys2 = psl_scratch_up(k->ctx, kp_off[K] ? keys2 : nullptr, 2 * nk, st, &e);
    A.depth2 = psl_scratch_up(k->ctx, kp_off[K] ? depth2 : nullptr, nk, st, &e);
    A.q = psl_scratch_up(k->ctx, nqmax ? queries : nullptr, rows, st, &e);
    A.idx1 = psl_scratch_up(k->ctx, nqmax ? idx1 : nullptr, rows, st, &e);
    A.qdesc = psl_scratch_up(k->ctx, nqmax ? qdesc : nullptr, rows * 32, st, &e);
    A.match = psl_scratch_up(k->ctx, (const int*)nullptr, rows, st, &e);
    A.status = psl_scratch_up(k->ctx, (const int*)nullptr, rows, st, &e);
    A.x3d = psl_scratch_up(k->ctx, (const float*)nullptr, rows * 3, st, &e);
    A.nmatches = psl_scratch_up(k->ctx, (const int*)nullptr, K, st, &e);
    A.created_by = psl_scratch_up(k->ctx, (const int*)nullptr, n1, st, &e);
    A.newp = psl_scratch_up(k->ctx, (const PslNewMapPoint*)nullptr, n1, st, &e);
    A.nnew = psl_scratch_up(k->ctx, (const int*)nullptr, 1, st, &e);
    A.geom = geom ? psl_scratch_up(k->ctx, (const PslMapPointGeom*)nullptr, n1, st, &e) : nullptr;
    A.obs_off = A.obs_kf = A.ref_kf = A.ref_level = nullptr;
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    PSL_HIP(hipMemsetAsync(A.newp, 0, n1 * sizeof(PslNewMapPoint), st));   // the rows behind *nnew come back as zeros
    if (geom) PSL_HIP(hipMemsetAsync(A.geom, 0, n1 * sizeof(PslMapPointGeom), st));
    if (int rc = new_points_launch(who, k, f2, A, kf1, N1, nb, K, fidx_off, kp_off, nq, nqmax, only_stereo, check_orientation, scale_factors,
                                   level_sigma2, nlevels))
        return rc;
    if (nqmax) {
        PSL_HIP(hipMemcpyAsync(match, A.match, rows * 4, hipMemcpyDeviceToHost, st));
        PSL_HIP(hipMemcpyAsync(status, A.status, rows * 4, hipMemcpyDeviceToHost, st));
        if (x3d) PSL_HIP(hipMemcpyAsync(x3d, A.x3d, rows * 12, hipMemcpyDeviceToHost, st));
    }
    PSL_HIP(hipMemcpyAsync(nmatches, A.nmatches, (size_t)K * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nnew, A.nnew, 4, hipMemcpyDeviceToHost, st));
    if (N1) {
        PSL_HIP(hipMemcpyAsync(created_by, A.created_by, (size_t)N1 * 4, hipMemcpyDeviceToHost, st));
        PSL_HIP(hipMemcpyAsync(newp, A.newp, (size_t)N1 * sizeof(PslNewMapPoint), hipMemcpyDeviceToHost, st));
        if (geom) PSL_HIP(hipMemcpyAsync(geom, A.geom, (size_t)N1 * sizeof(PslMapPointGeom), hipMemcpyDeviceToHost, st));
    }
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_line_fuse_best(pslfe_kf* k, const PslKeyLine* kls, int n, const uint8_t* desc, int ndesc, const PslLineFuseQuery* queries,
                            const uint8_t* qdesc, int nq, int32_t* best_idx, int32_t* best_dist) {
    PSL_REQUIRE(k && (nq == 0 || (queries && qdesc && best_idx && best_dist)) && (n == 0 || kls) && (ndesc == 0 || desc), PSLFE_E_INVALID,
                "pslfe_kf_line_fuse_best: NULL argument");
    PSL_REQUIRE(nq >= 0 && n >= 0 && n <= 0xffff && ndesc >= 0, PSLFE_E_INVALID, "pslfe_kf_line_fuse_best: bad count");
    if (nq == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    const size_t nn = (size_t)(n > 0 ? n : 1), nd = (size_t)(ndesc > 0 ? ndesc : 1);
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    PslKeyLine* d_kl = psl_scratch_up(k->ctx, n > 0 ? kls : nullptr, nn, st, &e);
    uint8_t* d_desc = psl_scratch_up(k->ctx, ndesc > 0 ? desc : nullptr, nd * 32, st, &e);
    PslLineFuseQuery* d_q = psl_scratch_up(k->ctx, queries, nq, st, &e);
    uint8_t* d_qd = psl_scratch_up(k->ctx, qdesc, (size_t)nq * 32, st, &e);
    int* d_i = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    int* d_d = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "pslfe_kf_line_fuse_best: %s", hipGetErrorString(e));
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.line_fuse");
        k_line_fuse_best<<<(nq + 3) / 4, 256, 0, st>>>(d_kl, n, d_desc, ndesc, d_q, d_qd, nq, d_i, d_d);
        PSL_STAGE_END(k->ctx, "kf.line_fuse");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(best_idx, d_i, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(best_dist, d_d, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_distinctive_descriptors(pslfe_kf* k, const uint8_t* desc, const int32_t* offsets, int npts, int32_t* best) {
    PSL_REQUIRE(k && (npts == 0 || (offsets && best)), PSLFE_E_INVALID, "pslfe_kf_distinctive_descriptors: NULL argument");
    PSL_REQUIRE(npts >= 0, PSLFE_E_INVALID, "pslfe_kf_distinctive_descriptors: npts = %d", npts);
    if (npts == 0) return PSLFE_OK;
    PSL_REQUIRE(offsets[0] == 0, PSLFE_E_INVALID, "pslfe_kf_distinctive_descriptors: offsets[0] must be 0");
    for (int p = 0; p < npts; ++p) {
        const int len = offsets[p + 1] - offsets[p];
        PSL_REQUIRE(len >= 0, PSLFE_E_INVALID, "pslfe_kf_distinctive_descriptors: offsets not ascending at %d", p);
        PSL_REQUIRE(len <= PSL_DISTINCT_MAX, PSLFE_E_CAPACITY, "pslfe_kf_distinctive_descriptors: point %d has %d observations (max %d)", p, len,
                    PSL_DISTINCT_MAX);
    }
    const size_t total = (size_t)offsets[npts];
    PSL_REQUIRE(total == 0 || desc, PSLFE_E_INVALID, "pslfe_kf_distinctive_descriptors: NULL descriptors");
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    uint8_t* d_desc = psl_scratch_up(k->ctx, total ? desc : nullptr, (total ? total : 1) * 32, st, &e);
    int* d_off = psl_scratch_up(k->ctx, offsets, (size_t)npts + 1, st, &e);
    int* d_best = psl_scratch_up(k->ctx, (const int*)nullptr, npts, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "pslfe_kf_distinctive_descriptors: %s", hipGetErrorString(e));
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.distinctive");
        k_distinctive<<<npts, 64, 0, st>>>(d_desc, d_off, npts, d_best);
        PSL_STAGE_END(k->ctx, "kf.distinctive");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(best, d_best, (size_t)npts * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

}  // extern "C"
