// libpslfe: the two ORBmatcher searches of LoopClosing::ComputeSim3 around SearchBySim3 (src/LoopClosing.cc:245-400). Product code.
// Reference behaviour reproduced:
//   ORBmatcher::SearchByBoW(pKF1, pKF2, vpMatches12)                     src/ORBmatcher.cc:522-655
//   ORBmatcher::SearchByProjection(pKF, Scw, vpPoints, vpMatched, th)    src/ORBmatcher.cc:290-403, after the projection
//   KeyFrame::GetFeaturesInArea                                           src/KeyFrame.cc:685-724
//
// SearchByBoW: vbMatched2 couples the queries of one vocabulary node (a feature lies in one node of a FeatureVector), nothing else,
// and candidates do not see each other: k_bow_kf_walk runs one wave per (candidate, node).  The node's KF2 descriptors are staged in
// LDS (9 words a row: 8 of descriptor, 1 of vbMatched2), lanes take the rows, (distance << 16 | row) keeps the first strict minimum
// and the second smallest distance through a wave-wide merge, and the wave walks the node's queries in order.  k_bow_kf_finish is the
// rotation histogram, one workgroup per candidate.
// SearchByProjection(pKF, Scw, ...): k_loop_proj_lists gives every map point, in parallel, its window candidates with distance <=
// TH_LOW that were free on entry, ascending by (distance, visiting order) - the only ones it can ever accept; k_loop_proj_resolve
// walks the map points in order, 64 at a time: a lane picks the first free keypoint of its list, the picks of the leading lanes that
// no lower lane disputes are final, the others pick again.  A map point whose cached entries are all gone while it has others (`more`)
// falls back to a window scan.
#include <limits.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "match_kernels.h"
#include "kf_project.h"

#define PSL_LOOP_TOPK 8
#define PSL_BOW_ROW_WORDS 9    // odd stride: lanes on consecutive rows hit different banks

struct BowGroup {   // the queries [q0, q0 + nq) of candidate `cand` share the run [start, start + len) (positions in the whole arrays)
    int cand, q0, nq, start, len;
};

struct BowKfArgs {
    FrameStore S;
    const int* slots;   // [ncand]
    const int* fidx;
    const BowGroup* groups;
    const PslBowQuery* q;
    const uint8_t* qdesc;
    const int* q_off;   // [ncand + 1]
    float nnratio;
    int check_ori;
    int* choice;
    int* match;
    int* nmatches;
};

// the candidate loop :554-619 for one (candidate, node): one wave
__global__ __launch_bounds__(64) void k_bow_kf_walk(BowKfArgs A) {
    extern __shared__ uint32_t s_row[];   // [len][PSL_BOW_ROW_WORDS]
    const int lane = threadIdx.x;
    const BowGroup G = A.groups[blockIdx.x];
    const FrameView V = psl_frame_view(A.S, A.slots[G.cand]);
    for (int j = lane; j < G.len; j += 64) {
        const int i2 = A.fidx[G.start + j];
        const bool ok = i2 >= 0 && i2 < V.n;
        uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
        if (ok) {
            d0 = *reinterpret_cast<const uint4*>(V.desc + (size_t)i2 * 8);
            d1 = *reinterpret_cast<const uint4*>(V.desc + (size_t)i2 * 8 + 4);
        }
        uint32_t* r = s_row + j * PSL_BOW_ROW_WORDS;
        r[0] = d0.x; r[1] = d0.y; r[2] = d0.z; r[3] = d0.w; r[4] = d1.x; r[5] = d1.y; r[6] = d1.z; r[7] = d1.w;
        r[8] = ok ? 0u : 1u;   // a row outside the slot can never be chosen
    }
    __syncthreads();
    const uint32_t* QD = reinterpret_cast<const uint32_t*>(A.qdesc);
    uint32_t nx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) nx[k] = G.nq > 0 ? QD[(size_t)G.q0 * 8 + k] : 0u;
    for (int t = 0; t < G.nq; ++t) {
        const int qi = G.q0 + t;
        uint32_t qd[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) qd[k] = nx[k];
        if (t + 1 < G.nq) {   // the next query's descriptor is on its way while this one is searched
#pragma unroll
            for (int k = 0; k < 8; ++k) nx[k] = QD[(size_t)(qi + 1) * 8 + k];
        }
        uint32_t k1 = PSL_KEY_INF, k2 = PSL_KEY_INF;
        for (int j = lane; j < G.len; j += 64) {
            const uint32_t* r = s_row + j * PSL_BOW_ROW_WORDS;
            if (r[8]) continue;   // vbMatched2[idx2] :576
            const int dist = psl_hamming256(qd, make_uint4(r[0], r[1], r[2], r[3]), make_uint4(r[4], r[5], r[6], r[7]));   // odd stride: scalar reads
            psl_merge2(k1, k2, ((uint32_t)dist << 16) | (uint32_t)j, PSL_KEY_INF);
        }
        psl_wave_min2(k1, k2);
        const int bestDist1 = k1 == PSL_KEY_INF ? 256 : (int)(k1 >> 16), bestDist2 = k2 == PSL_KEY_INF ? 256 : (int)(k2 >> 16);
        const bool acc = bestDist1 < PSL_TH_LOW && (float)bestDist1 < PSL_FMUL(A.nnratio, (float)bestDist2);   // :598-600
        const int pos = (int)(k1 & 0xffffu);
        if (lane == 0) {
            A.choice[qi] = acc ? A.fidx[G.start + pos] : -1;
            if (acc) s_row[pos * PSL_BOW_ROW_WORDS + 8] = 1u;   // vbMatched2[bestIdx2] = true :603
        }
        __syncthreads();
    }
}

// rotation histogram + ComputeThreeMaxima + outputs (:605-615, :634-652) of one candidate
__global__ __launch_bounds__(256) void k_bow_kf_finish(BowKfArgs A) {
    __shared__ int s_hist[PSL_HISTO];
    __shared__ int s_ind[3];
    __shared__ int s_nm;
    const int tid = threadIdx.x, c = blockIdx.x;
    const int q0 = A.q_off[c], q1 = A.q_off[c + 1];
    const FrameView V = psl_frame_view(A.S, A.slots[c]);
    if (tid < PSL_HISTO) s_hist[tid] = 0;
    if (tid == 0) { s_ind[0] = s_ind[1] = s_ind[2] = -1; s_nm = 0; }
    __syncthreads();
    if (A.check_ori) {
        for (int qi = q0 + tid; qi < q1; qi += 256) {
            const int c2 = A.choice[qi];
            if (c2 >= 0) atomicAdd(&s_hist[psl_rot_bin(A.q[qi].angle, V.kps[c2].angle)], 1);
        }
        __syncthreads();
        if (tid == 0) psl_three_maxima(s_hist, s_ind);
        __syncthreads();
    }
    int local = 0;
    for (int qi = q0 + tid; qi < q1; qi += 256) {
        const int c2 = A.choice[qi];
        bool good = c2 >= 0;
        if (good && A.check_ori) good = psl_rot_keep(psl_rot_bin(A.q[qi].angle, V.kps[c2].angle), s_ind);
        A.match[qi] = good ? c2 : -1;
        local += good;
    }
    local = psl_wave_sum(local);
    if ((tid & 63) == 0 && local) atomicAdd(&s_nm, local);
    __syncthreads();
    if (tid == 0) A.nmatches[c] = s_nm;
}

struct LoopProjArgs {
    FrameStore S;
    int slot;
    const PslProjQuery* q;
    const uint8_t* qdesc;
    int nq;
    const uint8_t* taken;   // [n] vpMatched[idx] != NULL on entry, or NULL
    int* topk;              // [nq][PSL_LOOP_TOPK] keypoints, -1 behind the last
    uint8_t* more;          // [nq] the query has candidates beyond its list
    int* match;
    int* assigned;          // [n], preset to -1
    int* nmatches;
};

// Key (distance << 16 | CSR position) of window candidate p for the loops of :372-392: octave band :380, free (`busy` == 0) :375,
// distance <= TH_LOW :394; PSL_KEY_INF otherwise.
template <typename Busy>
__device__ __forceinline__ uint32_t psl_loop_key(const FrameView& V, const PslProjQuery& q, const uint32_t (&qd)[8], int p, Busy busy) {
    if (p < 0) return PSL_KEY_INF;
    const int i2 = V.gidx[p];
    if (i2 < 0 || i2 >= V.n) return PSL_KEY_INF;
    const float2 xy = *reinterpret_cast<const float2*>(&V.kps[i2].x);
    const int octave = V.kps[i2].octave;
    const float r = q.radius;
    if (!(__builtin_fabsf(PSL_FSUB(xy.x, q.u)) < r && __builtin_fabsf(PSL_FSUB(xy.y, q.v)) < r)) return PSL_KEY_INF;
    if (octave < q.max_level - 1 || octave > q.max_level) return PSL_KEY_INF;
    if (busy(i2)) return PSL_KEY_INF;
    const int dist = psl_hamming256(qd, V.desc + (size_t)i2 * 8);
    return dist <= PSL_TH_LOW ? (((uint32_t)dist << 16) | (uint32_t)p) : PSL_KEY_INF;
}

// one wave per map point: its acceptable candidates, best first
__global__ __launch_bounds__(256) void k_loop_proj_lists(LoopProjArgs A) {
    const int qi = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (qi >= A.nq) return;
    int* out = A.topk + (size_t)qi * PSL_LOOP_TOPK;
    const PslProjQuery q = A.q[qi];
    if (!(q.radius >= 0)) {
        if (lane < PSL_LOOP_TOPK) out[lane] = -1;
        if (lane == 0) A.more[qi] = 0;
        return;
    }
    const FrameView V = psl_frame_view(A.S, A.slot);
    const uint32_t* QD = reinterpret_cast<const uint32_t*>(A.qdesc + (size_t)qi * 32);
    uint32_t qd[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) qd[k] = QD[k];
    const WindowCols W = psl_window_cols(V, q, nullptr);
    const uint8_t* taken = A.taken;
    uint32_t t[4] = {PSL_KEY_INF, PSL_KEY_INF, PSL_KEY_INF, PSL_KEY_INF};   // the lane's four smallest keys, ascending
    int cnt = 0;
    for (int base = 0; base < W.T; base += 64) {
        const int p = psl_window_pos(W, base + lane);
        const uint32_t key = psl_loop_key(V, q, qd, p, [taken](int i2) { return taken && taken[i2]; });
        if (key == PSL_KEY_INF) continue;
        ++cnt;
        psl_top4_insert(t, key);
    }
    int popped = 0, nout = 0, mine = -1;
    for (int k = 0; k < PSL_LOOP_TOPK; ++k) {
        if (__any(popped == 4 && cnt > 4)) break;   // a lane has keys this wave no longer sees: the list ends here, `more` is set
        const uint32_t m = psl_wave_min_u32(t[0]);
        if (m == PSL_KEY_INF) break;
        if (t[0] == m) { t[0] = t[1]; t[1] = t[2]; t[2] = t[3]; t[3] = PSL_KEY_INF; ++popped; }   // positions are distinct: one owner
        if (lane == k) mine = V.gidx[m & 0xffffu];
        ++nout;
    }
    const int total = psl_wave_sum(cnt);
    if (lane < PSL_LOOP_TOPK) out[lane] = lane < nout ? mine : -1;
    if (lane == 0) A.more[qi] = total > nout;
}

// the map points in order (:312-400): one wave, 64 map points at a time
__global__ __launch_bounds__(64) void k_loop_proj_resolve(LoopProjArgs A) {
    __shared__ uint8_t s_busy[PSL_QMAX];   // vpMatched[idx] != NULL
    __shared__ int s_claim[PSL_QMAX];      // lowest lane of the round that picks the keypoint
    const int lane = threadIdx.x;
    const FrameView V = psl_frame_view(A.S, A.slot);
    for (int i = lane; i < PSL_QMAX; i += 64) {
        s_busy[i] = (A.taken && i < V.n && A.taken[i]) ? 1 : 0;
        s_claim[i] = INT_MAX;
    }
    __syncthreads();
    int nm = 0;
    for (int base = 0; base < A.nq; base += 64) {
        const int qi = base + lane, cnt = min(64, A.nq - base);
        const bool active = lane < cnt;
        int e[PSL_LOOP_TOPK];
#pragma unroll
        for (int k = 0; k < PSL_LOOP_TOPK; ++k) e[k] = -1;
        bool more = false;
        if (active) {
            const int4 a = *reinterpret_cast<const int4*>(A.topk + (size_t)qi * PSL_LOOP_TOPK);
            const int4 b = *reinterpret_cast<const int4*>(A.topk + (size_t)qi * PSL_LOOP_TOPK + 4);
            e[0] = a.x; e[1] = a.y; e[2] = a.z; e[3] = a.w; e[4] = b.x; e[5] = b.y; e[6] = b.z; e[7] = b.w;
            more = A.more[qi] != 0;
        }
        int result = -1, done = 0;   // lanes below `done` are final
        while (done < cnt) {
            const bool open = active && lane >= done;
            int pick = -1;
            bool ended = false;
            if (open) {
#pragma unroll
                for (int k = 0; k < PSL_LOOP_TOPK; ++k) {
                    if (pick < 0 && !ended) {
                        if (e[k] < 0) ended = true;
                        else if (!s_busy[e[k]]) pick = e[k];
                    }
                }
            }
            // every cached candidate is gone and there are others - behind a full list, or behind one that k_loop_proj_lists cut short
            const bool rescan = open && pick < 0 && more;
            if (pick >= 0) atomicMin(&s_claim[pick], lane);
            __syncthreads();
            const bool bad = open && (rescan || (pick >= 0 && s_claim[pick] != lane));
            const unsigned long long bm = __ballot(bad);
            const int firstbad = bm ? __ffsll((long long)bm) - 1 : cnt;
            __syncthreads();
            if (pick >= 0) s_claim[pick] = INT_MAX;
            if (open && lane < firstbad) {   // every lower lane is final and none of them wants this keypoint
                result = pick;
                if (pick >= 0) { s_busy[pick] = 1; A.assigned[pick] = qi; }
            }
            done = firstbad;
            __syncthreads();
            if (done < cnt && __shfl((int)rescan, done)) {   // the wave scans the window of map point base + done against s_busy
                const int qs = base + done;
                const PslProjQuery q = A.q[qs];
                const uint32_t* QD = reinterpret_cast<const uint32_t*>(A.qdesc + (size_t)qs * 32);
                uint32_t qd[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) qd[k] = QD[k];
                const WindowCols W = psl_window_cols(V, q, nullptr);
                uint32_t best = PSL_KEY_INF;
                for (int b0 = 0; b0 < W.T; b0 += 64) {
                    const int p = psl_window_pos(W, b0 + lane);
                    best = min(best, psl_loop_key(V, q, qd, p, [&](int i2) { return s_busy[i2] != 0; }));
                }
                best = psl_wave_min_u32(best);
                const int kp = best == PSL_KEY_INF ? -1 : V.gidx[best & 0xffffu];
                if (lane == done) {
                    result = kp;
                    if (kp >= 0) { s_busy[kp] = 1; A.assigned[kp] = qs; }
                }
                ++done;
                __syncthreads();
            }
        }
        if (active) {
            A.match[qi] = result;
            nm += result >= 0;
        }
    }
    nm = psl_wave_sum(nm);
    if (lane == 0) *A.nmatches = nm;
}

// ---------------------------------------------------------------------------------------------
namespace {
int loop_check_slot(pslfe_frame* f, int slot, const char* who) {
    PSL_REQUIRE(slot >= 0 && slot < f->max_frames && f->slot_set[slot], PSLFE_E_STATE, "%s: slot %d not set", who, slot);
    return PSLFE_OK;
}

// SearchByProjection(pKF, Scw, ...) from :362 on.  The rows are the caller's (`queries`, host) or, with P != NULL, projected here from
// view / mp / skip (pslfe_kf_project, mode 1) and copied to queries_out when that is not NULL.
int loop_proj_search(pslfe_kf* k, pslfe_frame* f, int slot, const PslProjQuery* queries, const ProjParams* P, const PslKfView* view,
                     const PslMapPointGeom* mp, const uint8_t* skip, const uint8_t* qdesc, int nq, const uint8_t* taken, int32_t* match,
                     int32_t* assigned, int* nmatches, PslProjQuery* queries_out, const char* who) {
    *nmatches = 0;
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    FrameMeta m;
    PSL_HIP(hipMemcpyAsync(&m, f->S.meta + slot, sizeof(m), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    const int n = std::min(std::max(m.n, 0), PSL_QMAX);
    if (assigned)
        for (int i = 0; i < n; ++i) assigned[i] = -1;
    if (nq == 0) return PSLFE_OK;
    const size_t nk = (size_t)(n > 0 ? n : 1);
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    LoopProjArgs A;
    A.S = f->S; A.slot = slot; A.nq = nq;
    if (P) {
        KfProjBuffers B;
        if (int rc = psl_kf_project_upload(k->ctx, *P, view, 1, mp, skip, nq, false, &B, who)) return rc;
        A.q = B.q;
    } else {
        A.q = psl_scratch_up(k->ctx, queries, nq, st, &e);
    }
    A.qdesc = psl_scratch_up(k->ctx, qdesc, (size_t)nq * 32, st, &e);
    A.taken = (taken && n > 0) ? psl_scratch_up(k->ctx, taken, nk, st, &e) : nullptr;
    A.topk = psl_scratch_up(k->ctx, (const int*)nullptr, (size_t)nq * PSL_LOOP_TOPK, st, &e);
    A.more = psl_scratch_up(k->ctx, (const uint8_t*)nullptr, nq, st, &e);
    A.match = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    A.assigned = psl_scratch_up(k->ctx, (const int*)nullptr, nk, st, &e);
    A.nmatches = psl_scratch_up(k->ctx, (const int*)nullptr, 1, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    PSL_HIP(hipMemsetAsync(A.assigned, 0xff, nk * 4, st));
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.projection_sim3");
        k_loop_proj_lists<<<(nq + 3) / 4, 256, 0, st>>>(A);
        k_loop_proj_resolve<<<1, 64, 0, st>>>(A);
        PSL_STAGE_END(k->ctx, "kf.projection_sim3");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(match, A.match, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    if (assigned && n > 0) PSL_HIP(hipMemcpyAsync(assigned, A.assigned, (size_t)n * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nmatches, A.nmatches, 4, hipMemcpyDeviceToHost, st));
    if (P && queries_out) PSL_HIP(hipMemcpyAsync(queries_out, A.q, (size_t)nq * sizeof(PslProjQuery), hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}
}  // namespace

extern "C" {

int pslfe_kf_search_by_bow_candidates(pslfe_kf* k, pslfe_frame* f2, const int32_t* slots2, int ncand, const int32_t* fidx2,
                                      const int32_t* fidx2_off, const PslBowQuery* queries, const uint8_t* qdesc, const int32_t* q_off,
                                      float nnratio, int check_orientation, int32_t* match, int32_t* nmatches) {
    static const char* who = "pslfe_kf_search_by_bow_candidates";
    PSL_REQUIRE(k && f2, PSLFE_E_INVALID, "%s: NULL handle", who);
    PSL_REQUIRE(ncand >= 0, PSLFE_E_INVALID, "%s: ncand = %d", who, ncand);
    if (ncand == 0) return PSLFE_OK;
    PSL_REQUIRE(slots2 && fidx2_off && q_off && nmatches, PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(fidx2_off[0] == 0 && q_off[0] == 0, PSLFE_E_INVALID, "%s: fidx2_off[0] and q_off[0] must be 0", who);
    for (int c = 0; c < ncand; ++c) {
        PSL_REQUIRE(fidx2_off[c + 1] >= fidx2_off[c] && q_off[c + 1] >= q_off[c], PSLFE_E_INVALID, "%s: offsets not ascending at candidate %d", who, c);
        PSL_REQUIRE(fidx2_off[c + 1] - fidx2_off[c] <= f2->cap, PSLFE_E_CAPACITY, "%s: candidate %d has %d feature-vector entries, capacity %d", who,
                    c, fidx2_off[c + 1] - fidx2_off[c], f2->cap);
        if (int rc = loop_check_slot(f2, slots2[c], who)) return rc;
        nmatches[c] = 0;
    }
    const int nf = fidx2_off[ncand], nq = q_off[ncand];
    PSL_REQUIRE((nf == 0 || fidx2) && (nq == 0 || (queries && qdesc && match)), PSLFE_E_INVALID, "%s: NULL argument", who);
    if (nq == 0) return PSLFE_OK;
    // a FeatureVector holds a feature once; the runs of two nodes do not overlap.  Both are what lets the nodes run side by side.
    std::vector<BowGroup> groups;
    std::vector<int> seen(f2->cap, -1);
    std::vector<std::pair<int, int>> runs;
    int max_len = 0;
    for (int c = 0; c < ncand; ++c) {
        const int f0 = fidx2_off[c], nfc = fidx2_off[c + 1] - f0;
        for (int i = 0; i < nfc; ++i) {
            const int v = fidx2[f0 + i];
            PSL_REQUIRE(v >= 0 && v < f2->cap, PSLFE_E_INVALID, "%s: candidate %d: feature index %d out of range", who, c, v);
            PSL_REQUIRE(seen[v] != c, PSLFE_E_INVALID, "%s: candidate %d: feature %d appears twice in fidx2", who, c, v);
            seen[v] = c;
        }
        runs.clear();
        for (int i = q_off[c]; i < q_off[c + 1]; ++i) {
            const PslBowQuery& q = queries[i];
            PSL_REQUIRE(q.start >= 0 && q.len >= 0 && q.start <= nfc && q.len <= nfc - q.start, PSLFE_E_INVALID,
                        "%s: query %d refers to entries %d..%d of %d", who, i, q.start, q.start + q.len, nfc);
            if (!groups.empty() && groups.back().cand == c && groups.back().start == f0 + q.start && groups.back().len == q.len) {
                ++groups.back().nq;
                continue;
            }
            groups.push_back(BowGroup{c, i, 1, f0 + q.start, q.len});
            if (q.len > 0) runs.push_back(std::make_pair(q.start, q.len));
            max_len = std::max(max_len, q.len);
        }
        std::sort(runs.begin(), runs.end());
        for (size_t i = 1; i < runs.size(); ++i)
            PSL_REQUIRE(runs[i - 1].first + runs[i - 1].second <= runs[i].first, PSLFE_E_INVALID,
                        "%s: candidate %d: the runs at %d and %d overlap or one node's queries are not consecutive", who, c, runs[i - 1].first,
                        runs[i].first);
    }
    PSL_HIP(hipSetDevice(k->ctx->device));
    hipStream_t st = k->ctx->stream;
    if (int rc = psl_scratch_begin(k->ctx)) return rc;
    hipError_t e = hipSuccess;
    BowKfArgs A;
    A.S = f2->S;
    A.slots = psl_scratch_up(k->ctx, slots2, ncand, st, &e);
    A.fidx = psl_scratch_up(k->ctx, nf > 0 ? fidx2 : nullptr, (size_t)(nf > 0 ? nf : 1), st, &e);
    A.groups = psl_scratch_up(k->ctx, groups.data(), groups.size(), st, &e);
    A.q = psl_scratch_up(k->ctx, queries, nq, st, &e);
    A.qdesc = psl_scratch_up(k->ctx, qdesc, (size_t)nq * 32, st, &e);
    A.q_off = psl_scratch_up(k->ctx, q_off, (size_t)ncand + 1, st, &e);
    A.nnratio = nnratio; A.check_ori = check_orientation;
    A.choice = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    A.match = psl_scratch_up(k->ctx, (const int*)nullptr, nq, st, &e);
    A.nmatches = psl_scratch_up(k->ctx, (const int*)nullptr, ncand, st, &e);
    PSL_REQUIRE(e == hipSuccess, PSLFE_E_HIP, "%s: %s", who, hipGetErrorString(e));
    const size_t lds = (size_t)std::max(max_len, 1) * PSL_BOW_ROW_WORDS * 4;   // <= 4096 rows: 144 KB of the CU's 160
    if (lds > 48 * 1024)
        PSL_HIP(hipFuncSetAttribute(reinterpret_cast<const void*>(k_bow_kf_walk), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    {
        PSL_STAGE_BEGIN(k->ctx, "kf.bow_candidates");
        k_bow_kf_walk<<<(unsigned)groups.size(), 64, lds, st>>>(A);
        k_bow_kf_finish<<<ncand, 256, 0, st>>>(A);
        PSL_STAGE_END(k->ctx, "kf.bow_candidates");
    }
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(match, A.match, (size_t)nq * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipMemcpyAsync(nmatches, A.nmatches, (size_t)ncand * 4, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}

int pslfe_kf_search_by_bow(pslfe_kf* k, pslfe_frame* f2, int slot2, const int32_t* fidx2, int nfidx2, const PslBowQuery* queries,
                           const uint8_t* qdesc, int nq, float nnratio, int check_orientation, int32_t* match, int* nmatches) {
    PSL_REQUIRE(k && f2 && nmatches, PSLFE_E_INVALID, "pslfe_kf_search_by_bow: NULL argument");
    PSL_REQUIRE(nq >= 0 && nfidx2 >= 0, PSLFE_E_INVALID, "pslfe_kf_search_by_bow: negative count");
    const int32_t slot = slot2, foff[2] = {0, nfidx2}, qoff[2] = {0, nq};
    int32_t nm = 0;
    const int rc = pslfe_kf_search_by_bow_candidates(k, f2, &slot, 1, fidx2, foff, queries, qdesc, qoff, nnratio, check_orientation, match, &nm);
    *nmatches = nm;
    return rc;
}

int pslfe_kf_search_by_projection_sim3(pslfe_kf* k, pslfe_frame* f, int slot, const PslProjQuery* queries, const uint8_t* qdesc, int nq,
                                       const uint8_t* taken, int32_t* match, int32_t* assigned, int* nmatches) {
    static const char* who = "pslfe_kf_search_by_projection_sim3";
    PSL_REQUIRE(k && f && nmatches && (nq == 0 || (queries && qdesc && match)), PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(nq >= 0, PSLFE_E_INVALID, "%s: nq = %d", who, nq);
    if (int rc = loop_check_slot(f, slot, who)) return rc;
    return loop_proj_search(k, f, slot, queries, nullptr, nullptr, nullptr, nullptr, qdesc, nq, taken, match, assigned, nmatches, nullptr, who);
}

int pslfe_kf_search_by_projection_sim3_pose(pslfe_kf* k, pslfe_frame* f, const PslKfView* view, const PslMapPointGeom* mp,
                                            const uint8_t* mpdesc, const uint8_t* skip, int M, const PslCamera* cam, float min_x,
                                            float min_y, float max_x, float max_y, const float* scale_factors, int nlevels,
                                            float log_scale_factor, float th, const uint8_t* taken, int32_t* match, int32_t* assigned,
                                            int* nmatches, PslProjQuery* queries) {
    static const char* who = "pslfe_kf_search_by_projection_sim3_pose";
    PSL_REQUIRE(k && f, PSLFE_E_INVALID, "%s: NULL handle", who);
    PSL_REQUIRE(view && nmatches && (M == 0 || (mp && mpdesc && match)), PSLFE_E_INVALID, "%s: NULL argument", who);
    PSL_REQUIRE(M >= 0, PSLFE_E_INVALID, "%s: M = %d", who, M);
    ProjParams P;
    if (int rc = psl_proj_params(&P, PSLFE_KF_PROJ_SCW, cam, min_x, min_y, max_x, max_y, scale_factors, nlevels, log_scale_factor, th, who))
        return rc;
    PSL_REQUIRE(view->slot >= 0 && view->slot < f->max_frames, PSLFE_E_INVALID, "%s: slot %d outside the store (0..%d)", who, view->slot,
                f->max_frames - 1);
    if (int rc = loop_check_slot(f, view->slot, who)) return rc;
    return loop_proj_search(k, f, view->slot, nullptr, &P, view, mp, skip, mpdesc, M, taken, match, assigned, nmatches, queries, who);
}

}  // extern "C"
