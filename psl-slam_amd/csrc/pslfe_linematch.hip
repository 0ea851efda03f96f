// libpslfe: grid-guided line matchers. Product code.
//   LineIterator                                  add_src/lineIterator.cpp:34-77
//   Frame::AssignFeaturesToGridForLine            src/Frame.cc:286-309
//   Frame::GetFeaturesInAreaForLine               src/Frame.cc:752-826
//   LSDmatcher::SearchByProjection(cur,last,th)   add_src/LSDmatcher.cpp:112-215  (mode 0)
//   LSDmatcher::SearchByProjection(F,MLs,..,th)   add_src/LSDmatcher.cpp:260-352  (mode 1)
// A frame holds <= a few hundred lines; one wave owns the frame.  Queries are processed in the
// reference's order (first-come-first-served on taken lines); for each query lane 0 assembles the
// candidate list exactly as GetFeaturesInAreaForLine does (3 probe points, de-duplicated, push order)
// and the 64 lanes evaluate the candidates in parallel (key = distance << 16 | list position).
// pslfe_line_search_by_projection_device runs the same device code for many pairs with the grid in LDS.
#include <math.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "pslfe_internal.h"
#include "psl_device_math.h"
#include "match_kernels.h"

#define PSL_LG_COLS 64
#define PSL_LG_ROWS 48
#define PSL_LG_CELLS (PSL_LG_COLS * PSL_LG_ROWS)
#define PSL_LINE_MAX 2048   // lines per frame handled by the matcher
#define PSL_LINE_TH 95      // hard-coded acceptance threshold (add_src/LSDmatcher.cpp:205, 342)

struct LineBres {  // add_src/lineIterator.cpp
    bool steep; double dx, dy, error; int maxX, ystep, y, x;
    __device__ void init(double x1, double y1, double x2, double y2) {
        steep = fabs(PSL_DSUB(y2, y1)) > fabs(PSL_DSUB(x2, x1));
        if (steep) { double t = x1; x1 = y1; y1 = t; t = x2; x2 = y2; y2 = t; }
        if (x1 > x2) { double t = x1; x1 = x2; x2 = t; t = y1; y1 = y2; y2 = t; }
        dx = PSL_DSUB(x2, x1); dy = fabs(PSL_DSUB(y2, y1));
        error = dx / 2.0; ystep = (y1 < y2) ? 1 : -1;
        x = (int)x1; y = (int)y1; maxX = (int)x2;
    }
    __device__ bool next(int* px, int* py) {
        if (x > maxX) return false;
        if (steep) { *px = y; *py = x; } else { *px = x; *py = y; }
        error = PSL_DSUB(error, dy);
        if (error < 0) { y += ystep; error = PSL_DADD(error, dx); }
        x++;
        return true;
    }
};

struct LineMatchArgs {
    const PslKeyLine* kls; const uint8_t* desc; const double* eq; const double* dir3d; int n;
    float minX, minY, invW, invH;
    const PslLineQuery* q; const uint8_t* qdesc; int nq;
    const uint8_t* taken; float nnratio; double cos_gate;
    int* gstart; int* gidx; int gcap;   // CSR scratch in HBM: start [CELLS+1], idx [gcap]
    int* match; int* assigned; int* nmatches;
};

// Grid views of the window search: the one-frame kernel's CSR in HBM and the batched kernels' ends in LDS.
struct GridCsr {
    const int* start; const int* idx; int cap;
    __device__ void run(int c0, int c1, int* e0, int* e1) const { *e0 = start[c0]; *e1 = min(start[c1 + 1], cap); }
    __device__ int at(int e) const { return idx[e]; }
};
struct GridLds {
    const int* end; const uint16_t* idx;  // end[c] = one past the last entry of cell c
    __device__ void run(int c0, int c1, int* e0, int* e1) const { *e0 = c0 ? end[c0 - 1] : 0; *e1 = end[c1]; }
    __device__ int at(int e) const { return idx[e]; }
};
// mode-1 direction of line i: dir3d rows (first - second, one-frame entry point) or mvLines3D rows, differenced here
template <bool L6>
__device__ __forceinline__ void line_dir(const double* d3, int i, double* f) {
    if (L6) {
        const double* L = d3 + 6 * (size_t)i;
        f[0] = PSL_DSUB(L[0], L[3]); f[1] = PSL_DSUB(L[1], L[4]); f[2] = PSL_DSUB(L[2], L[5]);
    } else {
        const double* L = d3 + 3 * (size_t)i;
        f[0] = L[0]; f[1] = L[1]; f[2] = L[2];
    }
}

// GetFeaturesInAreaForLine src/Frame.cc:752-826, literal, on the calling lane: candidates in probe -> ix -> iy -> cell order,
// de-duplicated, a line rejected at one probe point tested again at the next.  Returns the candidate count.
template <typename Grid>
__device__ int line_candidates(const Grid& G, const PslKeyLine* kls, const double* eq, int n, float minX, float minY, float invW, float invH,
                               const PslLineQuery& q, uint16_t* s_cand, uint32_t* s_seen) {
    for (int w = 0; w < (n + 31) / 32; ++w) s_seen[w] = 0;
    int nc = 0;
    const float xs[3] = {q.x1, (float)((double)PSL_FADD(q.x1, q.x2) / 2.0), q.x2};
    const float ys[3] = {q.y1, (float)((double)PSL_FADD(q.y1, q.y2) / 2.0), q.y2};
    float d1x = PSL_FSUB(q.x1, q.x2), d1y = PSL_FSUB(q.y1, q.y2);
    const float n1 = sqrtf(PSL_FADD(PSL_FMUL(d1x, d1x), PSL_FMUL(d1y, d1y)));
    d1x = PSL_FDIV(d1x, n1); d1y = PSL_FDIV(d1y, n1);
    const float r = q.radius;
    for (int p = 0; p < 3; ++p) {
        const int minCX = max(0, (int)__builtin_floorf(PSL_FMUL(PSL_FSUB(PSL_FSUB(xs[p], minX), r), invW)));
        if (minCX >= PSL_LG_COLS) continue;
        const int maxCX = min(PSL_LG_COLS - 1, (int)__builtin_ceilf(PSL_FMUL(PSL_FADD(PSL_FSUB(xs[p], minX), r), invW)));
        if (maxCX < 0) continue;
        const int minCY = max(0, (int)__builtin_floorf(PSL_FMUL(PSL_FSUB(PSL_FSUB(ys[p], minY), r), invH)));
        if (minCY >= PSL_LG_ROWS) continue;
        const int maxCY = min(PSL_LG_ROWS - 1, (int)__builtin_ceilf(PSL_FMUL(PSL_FADD(PSL_FSUB(ys[p], minY), r), invH)));
        if (maxCY < 0) continue;
        for (int ix = minCX; ix <= maxCX; ++ix) {
            int e0, e1;
            G.run(ix * PSL_LG_ROWS + minCY, ix * PSL_LG_ROWS + maxCY, &e0, &e1);
            for (int e = e0; e < e1; ++e) {
                const int j = G.at(e);
                if ((s_seen[j >> 5] >> (j & 31)) & 1u) continue;
                float d2x = PSL_FSUB(kls[j].startPointX, kls[j].endPointX), d2y = PSL_FSUB(kls[j].startPointY, kls[j].endPointY);
                const float n2 = sqrtf(PSL_FADD(PSL_FMUL(d2x, d2x), PSL_FMUL(d2y, d2y)));
                d2x = PSL_FDIV(d2x, n2); d2y = PSL_FDIV(d2y, n2);
                const float cosS = __builtin_fabsf(PSL_FADD(PSL_FMUL(d1x, d2x), PSL_FMUL(d1y, d2y)));
                if (cosS < q.th_cos) continue;
                const float dist = (float)PSL_DADD(PSL_DADD(PSL_DMUL(eq[3 * j], (double)xs[p]), PSL_DMUL(eq[3 * j + 1], (double)ys[p])), eq[3 * j + 2]);
                if (__builtin_fabsf(dist) < r) { s_cand[nc++] = (uint16_t)j; s_seen[j >> 5] |= 1u << (j & 31); }
            }
        }
    }
    return nc;
}

// The 64 lanes evaluate the candidates (key = distance << 16 | list position) and pick as the reference's loop does
// (:165-213 / :296-349).  All lanes return the pick.
template <int MODE, bool L6>
__device__ int line_pick(const PslKeyLine* kls, const uint8_t* desc, const double* d3, const PslLineQuery& q, const uint8_t* qdesc,
                         const uint16_t* s_cand, int nc, const uint8_t* s_blocked, double cos_gate, float nnratio) {
    const int lane = threadIdx.x;
    uint32_t k1 = 0xffffffffu, k2 = 0xffffffffu;
    uint32_t qd[8];
    const uint32_t* QD = reinterpret_cast<const uint32_t*>(qdesc);
#pragma unroll
    for (int k = 0; k < 8; ++k) qd[k] = QD[k];
    for (int ci = lane; ci < nc; ci += 64) {
        const int i2 = s_cand[ci];
        if (s_blocked[i2]) continue;
        const PslKeyLine kl = kls[i2];
        if (MODE == 0) {
            const double vc0 = (double)PSL_FSUB(kl.ePointInOctaveX, kl.sPointInOctaveX), vc1 = (double)PSL_FSUB(kl.ePointInOctaveY, kl.sPointInOctaveY);
            const double vl0 = (double)q.vx, vl1 = (double)q.vy;
            const double dot = PSL_DADD(PSL_DMUL(vc0, vl0), PSL_DMUL(vc1, vl1));
            const double den = PSL_DMUL(__dsqrt_rn(PSL_DADD(PSL_DMUL(vc0, vc0), PSL_DMUL(vc1, vc1))), __dsqrt_rn(PSL_DADD(PSL_DMUL(vl0, vl0), PSL_DMUL(vl1, vl1))));
            if (fabs(dot / den) < cos_gate) continue;
            const float mx = fmaxf(q.length, kl.lineLength), mn = fminf(q.length, kl.lineLength);
            if ((double)PSL_FDIV(mn, mx) < 0.75) continue;
        } else {
            double f[3];
            line_dir<L6>(d3, i2, f);
            const float dot = (float)PSL_DADD(PSL_DADD(PSL_DMUL(f[0], q.wdir[0]), PSL_DMUL(f[1], q.wdir[1])), PSL_DMUL(f[2], q.wdir[2]));
            const float mag_f = (float)__dsqrt_rn(PSL_DADD(PSL_DADD(PSL_DMUL(f[0], f[0]), PSL_DMUL(f[1], f[1])), PSL_DMUL(f[2], f[2])));
            const float mag_ml = (float)__dsqrt_rn(PSL_DADD(PSL_DADD(PSL_DMUL(q.wdir[0], q.wdir[0]), PSL_DMUL(q.wdir[1], q.wdir[1])), PSL_DMUL(q.wdir[2], q.wdir[2])));
            const float angle = __builtin_fabsf(PSL_FDIV(dot, PSL_FMUL(mag_f, mag_ml)));
            if ((double)angle < cos_gate) continue;
        }
        const uint32_t* D = reinterpret_cast<const uint32_t*>(desc) + (size_t)i2 * 8;
        int d = 0;
#pragma unroll
        for (int k = 0; k < 8; ++k) d += __popc(qd[k] ^ D[k]);   // rows of a caller's array: no 16-byte alignment assumed
        const uint32_t key = ((uint32_t)d << 16) | (uint32_t)ci;
        if (key < k1) { k2 = k1; k1 = key; } else if (key < k2) k2 = key;
    }
    psl_wave_min2(k1, k2);
    int pick = -1;
    if (k1 != 0xffffffffu && (int)(k1 >> 16) <= PSL_LINE_TH) {
        pick = s_cand[k1 & 0xffff];
        // the reference's bestDist2 starts at 256 and moves only on dist < bestDist2 (:296-340): a candidate at 256 is never the second best
        if (MODE == 1 && k2 != 0xffffffffu && (k2 >> 16) < 256) {
            const int l1 = kls[pick].octave, l2 = kls[s_cand[k2 & 0xffff]].octave;
            if (l1 == l2 && (float)(k1 >> 16) > PSL_FMUL(nnratio, (float)(k2 >> 16))) pick = -1;
        }
    }
    return pick;
}

template <int MODE>
__global__ __launch_bounds__(64) void k_line_proj_match(LineMatchArgs A) {
    __shared__ int s_cnt[PSL_LG_CELLS + 1];
    __shared__ int s_owner[PSL_LINE_MAX];
    __shared__ uint8_t s_blocked[PSL_LINE_MAX];
    __shared__ uint16_t s_cand[PSL_LINE_MAX];
    __shared__ uint32_t s_seen[PSL_LINE_MAX / 32];
    __shared__ int s_ncand;
    const int lane = threadIdx.x;
    const int n = A.n < PSL_LINE_MAX ? A.n : PSL_LINE_MAX;
    // ---- AssignFeaturesToGridForLine: count, scan, fill, sort (lists end up ascending by line index)
    for (int c = lane; c <= PSL_LG_CELLS; c += 64) s_cnt[c] = 0;
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < n; i += 64) {
        LineBres it;
        it.init((double)PSL_FMUL(A.kls[i].startPointX, A.invW), (double)PSL_FMUL(A.kls[i].startPointY, A.invH),
                (double)PSL_FMUL(A.kls[i].endPointX, A.invW), (double)PSL_FMUL(A.kls[i].endPointY, A.invH));
        int px, py;
        while (it.next(&px, &py))
            if (px >= 0 && px < PSL_LG_COLS && py >= 0 && py < PSL_LG_ROWS) atomicAdd(&s_cnt[px * PSL_LG_ROWS + py], 1);
    }
    __builtin_amdgcn_wave_barrier();
    if (lane == 0) {
        int acc = 0;
        for (int c = 0; c < PSL_LG_CELLS; ++c) { const int t = s_cnt[c]; s_cnt[c] = acc; A.gstart[c] = acc; acc += t; }
        s_cnt[PSL_LG_CELLS] = acc; A.gstart[PSL_LG_CELLS] = acc;
    }
    __builtin_amdgcn_wave_barrier();
    for (int i = lane; i < n; i += 64) {
        LineBres it;
        it.init((double)PSL_FMUL(A.kls[i].startPointX, A.invW), (double)PSL_FMUL(A.kls[i].startPointY, A.invH),
                (double)PSL_FMUL(A.kls[i].endPointX, A.invW), (double)PSL_FMUL(A.kls[i].endPointY, A.invH));
        int px, py;
        while (it.next(&px, &py))
            if (px >= 0 && px < PSL_LG_COLS && py >= 0 && py < PSL_LG_ROWS) {
                const int p = atomicAdd(&s_cnt[px * PSL_LG_ROWS + py], 1);
                if (p < A.gcap) A.gidx[p] = i;
            }
    }
    __builtin_amdgcn_wave_barrier();
    for (int c = lane; c < PSL_LG_CELLS; c += 64) {  // s_cnt[c] is now the END of cell c; start from gstart
        const int lo = A.gstart[c], hi = min(s_cnt[c], A.gcap);
        for (int i = lo + 1; i < hi; ++i) {
            const int v = A.gidx[i];
            int j = i - 1;
            while (j >= lo && A.gidx[j] > v) { A.gidx[j + 1] = A.gidx[j]; --j; }
            A.gidx[j + 1] = v;
        }
    }
    for (int i = lane; i < n; i += 64) { s_owner[i] = -1; s_blocked[i] = (A.taken && A.taken[i]) ? 1 : 0; }
    __builtin_amdgcn_wave_barrier();

    const GridCsr G = {A.gstart, A.gidx, A.gcap};
    int nmatches = 0;
    for (int qi = 0; qi < A.nq; ++qi) {
        const PslLineQuery q = A.q[qi];
        if (lane == 0) s_ncand = line_candidates(G, A.kls, A.eq, n, A.minX, A.minY, A.invW, A.invH, q, s_cand, s_seen);
        __builtin_amdgcn_wave_barrier();
        const int pick = line_pick<MODE, false>(A.kls, A.desc, A.dir3d, q, A.qdesc + (size_t)qi * 32, s_cand, s_ncand, s_blocked,
                                                A.cos_gate, A.nnratio);
        if (lane == 0) {
            A.match[qi] = pick;
            if (pick >= 0) { s_owner[pick] = qi; s_blocked[pick] = q.blocks != 0; }
        }
        nmatches += pick >= 0;
        __builtin_amdgcn_wave_barrier();
    }
    if (A.assigned) for (int i = lane; i < n; i += 64) A.assigned[i] = s_owner[i];
    if (lane == 0) *A.nmatches = nmatches;
}

// ---- Batched form: one 64-lane workgroup per pair, the grid in LDS.
// LDS of the first launch: cell ends 12 KB + 8192 16-bit entries 16 KB + per-line state 7 KB = 36 KB -> 4 workgroups (waves) per CU.
// A pair whose grid has more entries goes to the second launch: 65536 entries (128 KB; a line adds at most 64 in-grid cells, so
// 1024 lines always fit), 148 KB of LDS, one workgroup per CU.
#define PSL_LGD_MAXN 1024
#define PSL_LGD_SMALL 8192
#define PSL_LGD_BIG (64 * PSL_LGD_MAXN)

struct LineBatchArgs {
    const PslKeyLine* kls; const uint8_t* desc; const double* eq; const int32_t* nkl; int kl_stride;
    const double* lines3d;  // [npairs][kl_stride][6] (mode 1)
    float minX, minY, invW, invH;
    const PslLineQuery* q; const uint8_t* qdesc; const int32_t* nq; int qstride;
    const uint8_t* taken; float nnratio; double cos_gate;
    int32_t* match; int32_t* assigned; int32_t* nmatches;
    int32_t* ovf_list; int32_t* ovf_count; int32_t* nfallback;
};

struct LineLds {
    int* end; uint16_t* idx; int* owner; uint8_t* blocked; uint16_t* cand; uint32_t* seen; int* ncand;
};

// The whole search of pair p.  Returns false (uniformly, before any output is written) when the grid needs more than ecap entries.
template <int MODE>
__device__ bool line_pair_search(const LineBatchArgs& A, int p, const LineLds& S, int ecap) {
    const int lane = threadIdx.x;
    const size_t base = (size_t)p * A.kl_stride;
    const PslKeyLine* kls = A.kls + base;
    const int n = min(A.nkl[p], A.kl_stride);
    // ---- AssignFeaturesToGridForLine: count, scan (lane l owns cells 48l..48l+47), fill, sort each cell ascending
    for (int c = lane; c < PSL_LG_CELLS; c += 64) S.end[c] = 0;
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        LineBres it;
        it.init((double)PSL_FMUL(kls[i].startPointX, A.invW), (double)PSL_FMUL(kls[i].startPointY, A.invH),
                (double)PSL_FMUL(kls[i].endPointX, A.invW), (double)PSL_FMUL(kls[i].endPointY, A.invH));
        int px, py;
        while (it.next(&px, &py))
            if (px >= 0 && px < PSL_LG_COLS && py >= 0 && py < PSL_LG_ROWS) atomicAdd(&S.end[px * PSL_LG_ROWS + py], 1);
    }
    __syncthreads();
    constexpr int PER = PSL_LG_CELLS / 64;
    int own = 0;
    for (int k = 0; k < PER; ++k) own += S.end[lane * PER + k];
    int incl = own;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(incl, o); if (lane >= o) incl += u; }
    const int total = __shfl(incl, 63);
    if (total > ecap) return false;
    int acc = incl - own;
    for (int k = 0; k < PER; ++k) { const int t = S.end[lane * PER + k]; S.end[lane * PER + k] = acc; acc += t; }
    __syncthreads();
    for (int i = lane; i < n; i += 64) {
        LineBres it;
        it.init((double)PSL_FMUL(kls[i].startPointX, A.invW), (double)PSL_FMUL(kls[i].startPointY, A.invH),
                (double)PSL_FMUL(kls[i].endPointX, A.invW), (double)PSL_FMUL(kls[i].endPointY, A.invH));
        int px, py;
        while (it.next(&px, &py))
            if (px >= 0 && px < PSL_LG_COLS && py >= 0 && py < PSL_LG_ROWS) S.idx[atomicAdd(&S.end[px * PSL_LG_ROWS + py], 1)] = (uint16_t)i;
    }
    __syncthreads();
    for (int c = lane; c < PSL_LG_CELLS; c += 64) {  // S.end[c] is now the end of cell c, S.end[c - 1] its start
        const int lo = c ? S.end[c - 1] : 0, hi = S.end[c];
        for (int i = lo + 1; i < hi; ++i) {
            const uint16_t v = S.idx[i];
            int j = i - 1;
            while (j >= lo && S.idx[j] > v) { S.idx[j + 1] = S.idx[j]; --j; }
            S.idx[j + 1] = v;
        }
    }
    const uint8_t* taken = A.taken ? A.taken + base : nullptr;
    for (int i = lane; i < n; i += 64) { S.owner[i] = -1; S.blocked[i] = (taken && taken[i]) ? 1 : 0; }
    __syncthreads();

    const GridLds G = {S.end, S.idx};
    const double* eq = A.eq + base * 3;
    const uint8_t* desc = A.desc + base * 32;
    const double* d3 = MODE == 1 ? A.lines3d + base * 6 : nullptr;
    const size_t qbase = (size_t)p * A.qstride;
    const int nq = min(A.nq[p], A.qstride);
    int nmatches = 0;
    for (int qi = 0; qi < nq; ++qi) {
        const PslLineQuery q = A.q[qbase + qi];
        if (lane == 0) *S.ncand = line_candidates(G, kls, eq, n, A.minX, A.minY, A.invW, A.invH, q, S.cand, S.seen);
        __syncthreads();
        const int pick = line_pick<MODE, true>(kls, desc, d3, q, A.qdesc + (qbase + qi) * 32, S.cand, *S.ncand, S.blocked, A.cos_gate,
                                               A.nnratio);
        if (lane == 0) {
            A.match[qbase + qi] = pick;
            if (pick >= 0) { S.owner[pick] = qi; S.blocked[pick] = q.blocks != 0; }
        }
        nmatches += pick >= 0;
        __syncthreads();
    }
    if (A.assigned) for (int i = lane; i < n; i += 64) A.assigned[base + i] = S.owner[i];
    if (lane == 0) A.nmatches[p] = nmatches;
    return true;
}

template <int MODE>
__global__ __launch_bounds__(64) void k_line_proj_match_batch(LineBatchArgs A) {
    __shared__ int s_end[PSL_LG_CELLS];
    __shared__ uint16_t s_idx[PSL_LGD_SMALL];
    __shared__ int s_owner[PSL_LGD_MAXN];
    __shared__ uint8_t s_blocked[PSL_LGD_MAXN];
    __shared__ uint16_t s_cand[PSL_LGD_MAXN];
    __shared__ uint32_t s_seen[PSL_LGD_MAXN / 32];
    __shared__ int s_ncand;
    const LineLds S = {s_end, s_idx, s_owner, s_blocked, s_cand, s_seen, &s_ncand};
    const int p = blockIdx.x;
    if (!line_pair_search<MODE>(A, p, S, PSL_LGD_SMALL) && threadIdx.x == 0) A.ovf_list[atomicAdd(A.ovf_count, 1)] = p;
}

// The pairs the first launch listed; a grid of at most one workgroup per CU walks the list.
template <int MODE>
__global__ __launch_bounds__(64) void k_line_proj_match_batch_big(LineBatchArgs A) {
    __shared__ int s_end[PSL_LG_CELLS];
    __shared__ uint16_t s_idx[PSL_LGD_BIG];
    __shared__ int s_owner[PSL_LGD_MAXN];
    __shared__ uint8_t s_blocked[PSL_LGD_MAXN];
    __shared__ uint16_t s_cand[PSL_LGD_MAXN];
    __shared__ uint32_t s_seen[PSL_LGD_MAXN / 32];
    __shared__ int s_ncand;
    const LineLds S = {s_end, s_idx, s_owner, s_blocked, s_cand, s_seen, &s_ncand};
    const int cnt = *A.ovf_count;
    for (int k = blockIdx.x; k < cnt; k += gridDim.x) {
        line_pair_search<MODE>(A, A.ovf_list[k], S, PSL_LGD_BIG);
        __syncthreads();
    }
    if (blockIdx.x == 0 && threadIdx.x == 0 && A.nfallback) *A.nfallback = cnt;
}

extern "C" {

int pslfe_line_search_by_projection(pslfe_ctx* ctx, const PslKeyLine* kls, const uint8_t* desc, const double* lineEq, const double* dir3d, int n,
                                    float min_x, float min_y, float max_x, float max_y, const PslLineQuery* queries, const uint8_t* qdesc,
                                    int nq, const uint8_t* taken, int mode, float nnratio, int32_t* match, int32_t* assigned, int* nmatches,
                                    int32_t* grid_start, int32_t* grid_idx, int grid_cap, int* grid_n) {
    PSL_REQUIRE(ctx && nmatches && (nq == 0 || (queries && qdesc && match)) && (n == 0 || (kls && desc && lineEq)), PSLFE_E_INVALID,
                "pslfe_line_search_by_projection: NULL argument");
    PSL_REQUIRE(mode == 0 || (mode == 1 && (n == 0 || dir3d)), PSLFE_E_INVALID, "pslfe_line_search_by_projection: mode %d", mode);
    PSL_REQUIRE(n >= 0 && n <= PSL_LINE_MAX && nq >= 0, PSLFE_E_CAPACITY, "pslfe_line_search_by_projection: %d lines (max %d)", n, PSL_LINE_MAX);
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "pslfe_line_search_by_projection: empty image bounds");
    *nmatches = 0;
    for (int i = 0; i < nq; ++i) match[i] = -1;
    if (assigned) for (int i = 0; i < n; ++i) assigned[i] = -1;
    if (n == 0) return PSLFE_OK;
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    { const int rc_ = psl_scratch_begin(ctx); if (rc_) return rc_; }
    hipError_t e = hipSuccess;
    LineMatchArgs A;
    memset(&A, 0, sizeof(A));
    A.kls = psl_scratch_up(ctx, kls, n, st, &e);
    A.desc = psl_scratch_up(ctx, desc, (size_t)n * 32, st, &e);
    A.eq = psl_scratch_up(ctx, lineEq, (size_t)n * 3, st, &e);
    A.dir3d = dir3d ? psl_scratch_up(ctx, dir3d, (size_t)n * 3, st, &e) : nullptr;
    A.n = n;
    A.minX = min_x; A.minY = min_y;
    A.invW = (float)PSL_LG_COLS / (float)(max_x - min_x);
    A.invH = (float)PSL_LG_ROWS / (float)(max_y - min_y);
    A.q = psl_scratch_up(ctx, queries, nq, st, &e);
    A.qdesc = psl_scratch_up(ctx, qdesc, (size_t)nq * 32, st, &e);
    A.nq = nq;
    A.taken = taken ? psl_scratch_up(ctx, taken, n, st, &e) : nullptr;
    A.nnratio = nnratio;
    A.cos_gate = mode == 0 ? cos(10.0 / 180.0 * M_PI) : cos(15.0 / 180.0 * M_PI);
    A.gcap = n * (PSL_LG_COLS + PSL_LG_ROWS);  // a Bresenham walk visits at most max(cols, rows) + 1 cells
    A.gstart = psl_scratch_up(ctx, (const int*)nullptr, PSL_LG_CELLS + 1, st, &e);
    A.gidx = psl_scratch_up(ctx, (const int*)nullptr, A.gcap, st, &e);
    A.match = psl_scratch_up(ctx, (const int*)nullptr, nq ? nq : 1, st, &e);
    A.assigned = psl_scratch_up(ctx, (const int*)nullptr, n, st, &e);
    A.nmatches = psl_scratch_up(ctx, (const int*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "pslfe_line_search_by_projection: %s", hipGetErrorString(e));
    {
        PSL_STAGE_BEGIN(ctx, "line.proj_match");
        if (mode == 0) k_line_proj_match<0><<<1, 64, 0, st>>>(A); else k_line_proj_match<1><<<1, 64, 0, st>>>(A);
        PSL_STAGE_END(ctx, "line.proj_match");
    }
    PSL_HIP(hipGetLastError());
    if (nq) PSL_HIP(hipMemcpyAsync(match, A.match, (size_t)nq * sizeof(int), hipMemcpyDeviceToHost, st));
    if (assigned) PSL_HIP(hipMemcpyAsync(assigned, A.assigned, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nmatches, A.nmatches, sizeof(int), hipMemcpyDeviceToHost, st));
    if (grid_start) PSL_HIP(hipMemcpyAsync(grid_start, A.gstart, (PSL_LG_CELLS + 1) * sizeof(int), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    if (grid_start && grid_n) *grid_n = grid_start[PSL_LG_CELLS];
    if (grid_start && grid_idx) {
        const int m = std::min(std::min(grid_start[PSL_LG_CELLS], grid_cap), A.gcap);
        if (m > 0) PSL_HIP(hipMemcpy(grid_idx, A.gidx, (size_t)m * sizeof(int), hipMemcpyDeviceToHost));
    }
    return PSLFE_OK;
}

int pslfe_line_search_by_projection_device(pslfe_ctx* ctx, int npairs, const PslKeyLine* d_kls, const uint8_t* d_desc, const double* d_lineEq,
                                           const int32_t* d_nkl, int kl_stride, const double* d_lines3d, int lines3d_stride, float min_x,
                                           float min_y, float max_x, float max_y, const PslLineQuery* d_queries, const uint8_t* d_qdesc,
                                           const int32_t* d_nq, int qstride, const uint8_t* d_taken, int mode, float nnratio,
                                           int32_t* d_match, int32_t* d_assigned, int32_t* d_nmatches, int32_t* d_nfallback) {
    static const char* what = "pslfe_line_search_by_projection_device";
    PSL_REQUIRE(mode == 0 || (mode == 1 && d_lines3d), PSLFE_E_INVALID, "%s: mode %d%s", what, mode, mode == 1 ? " without mvLines3D" : "");
    PSL_REQUIRE(mode == 0 || lines3d_stride == kl_stride, PSLFE_E_INVALID, "%s: mvLines3D stride %d != keyline stride %d", what,
                lines3d_stride, kl_stride);
    PSL_REQUIRE(npairs >= 1 && kl_stride >= 1 && qstride >= 1, PSLFE_E_INVALID, "%s: npairs %d kl_stride %d qstride %d", what, npairs,
                kl_stride, qstride);
    PSL_REQUIRE(kl_stride <= PSL_LGD_MAXN, PSLFE_E_CAPACITY, "%s: kl_stride %d (max %d)", what, kl_stride, PSL_LGD_MAXN);
    PSL_REQUIRE(max_x > min_x && max_y > min_y, PSLFE_E_INVALID, "%s: empty image bounds", what);
    PSL_REQUIRE(ctx && d_kls && d_desc && d_lineEq && d_nkl && d_queries && d_qdesc && d_nq && d_match && d_nmatches, PSLFE_E_INVALID,
                "%s: NULL argument", what);
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    { const int rc_ = psl_scratch_begin(ctx); if (rc_) return rc_; }
    hipError_t e = hipSuccess;
    int32_t* ovf = psl_scratch_up<int32_t>(ctx, nullptr, (size_t)npairs + 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: scratch: %s", what, hipGetErrorString(e));
    PSL_HIP(hipMemsetAsync(ovf, 0, sizeof(int32_t), st));
    LineBatchArgs A;
    memset(&A, 0, sizeof(A));
    A.kls = d_kls; A.desc = d_desc; A.eq = d_lineEq; A.nkl = d_nkl; A.kl_stride = kl_stride;
    A.lines3d = mode == 1 ? d_lines3d : nullptr;
    A.minX = min_x; A.minY = min_y;
    A.invW = (float)PSL_LG_COLS / (float)(max_x - min_x);
    A.invH = (float)PSL_LG_ROWS / (float)(max_y - min_y);
    A.q = d_queries; A.qdesc = d_qdesc; A.nq = d_nq; A.qstride = qstride;
    A.taken = d_taken; A.nnratio = nnratio;
    A.cos_gate = mode == 0 ? cos(10.0 / 180.0 * M_PI) : cos(15.0 / 180.0 * M_PI);
    A.match = d_match; A.assigned = d_assigned; A.nmatches = d_nmatches;
    A.ovf_count = ovf; A.ovf_list = ovf + 1; A.nfallback = d_nfallback;
    const int nbig = std::min(npairs, ctx->cu_count > 0 ? ctx->cu_count : 256);
    {
        PSL_STAGE_BEGIN(ctx, "line.proj_match_batch");
        if (mode == 0) {
            k_line_proj_match_batch<0><<<npairs, 64, 0, st>>>(A);
            k_line_proj_match_batch_big<0><<<nbig, 64, 0, st>>>(A);
        } else {
            k_line_proj_match_batch<1><<<npairs, 64, 0, st>>>(A);
            k_line_proj_match_batch_big<1><<<nbig, 64, 0, st>>>(A);
        }
        PSL_STAGE_END(ctx, "line.proj_match_batch");
    }
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

}  // extern "C"
