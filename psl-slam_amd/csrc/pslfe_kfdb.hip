// libpslfe: the keyframe database of loop closing and relocalisation on the device. Product code.
// Reference behaviour reproduced: KeyFrameDatabase::add / erase / clear src/KeyFrameDatabase.cc:40-73, the inverted-file walk and
// the scores of DetectLoopCandidates :76-139 and DetectRelocalizationCandidates :199-253, the minScore loop of
// LoopClosing::DetectLoop src/LoopClosing.cc:124-138, DBoW2::L1Scoring::score Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68.
// The covisibility tails (:141-196, :255-308) stay with the host mirrors: they walk the caller's map graph.
//
// The reference keeps an inverted file (word -> list of keyframes) and scores the keyframes that a walk over the query's words
// reaches.  Here the BowVectors themselves are resident, one fixed-stride row of ascending (word id, value) pairs per slot, and
// a query visits every live row: k_kfdb_query, one wave per (slot, query).  The query's pairs are staged once per workgroup in
// LDS; the lanes take 64 row entries at a time and binary-search the query ids; the ballot of the hits gives the number of common
// words, its lowest set lane the first common word, and the score adds the hit lanes' terms in lane order, which inside a chunk
// is ascending word order, chunk after chunk: the additions of L1Scoring::score in its order, so the f64 result is the same bits.
// What the walk leaves per keyframe (mnLoopWords / mnRelocWords, its place in lKFsSharingWords) follows from the number of
// common words, the smallest common word and the order of the adds, which the handle keeps on the host.
#include <string.h>

#include <algorithm>
#include <vector>

#include "pslfe_internal.h"

#define PSL_BOW_NMAX 4096       // the row limit of k_bow_vectors (pslfe_bow.hip): no BowVector is longer
#define PSL_KFDB_WAVES 4        // waves per workgroup
#define PSL_KFDB_MAX_SPB 64     // slots per workgroup, at most (a multiple of PSL_KFDB_WAVES)

// One wave per (row, query); a workgroup stages its query once and walks `spb` rows.  rows: nrows = max_keyframes and
// slots == nullptr (every slot; dead or excluded ones get zeros), or the nrows slots of `slots` (score-only: no exclusion, words /
// first_word / max_common may be nullptr).  Outputs at [query][row].
__global__ __launch_bounds__(PSL_KFDB_WAVES * 64) void k_kfdb_query(
    const int32_t* __restrict__ row_id, const double* __restrict__ row_val, const int32_t* __restrict__ row_len, const int32_t* __restrict__ row_live,
    int row_stride, int max_kf, int nrows, const int32_t* __restrict__ slots, const int32_t* __restrict__ q_id, const double* __restrict__ q_val,
    const int32_t* __restrict__ q_n, int qstride, int qcap, const uint8_t* __restrict__ exclude, int spb, int32_t* __restrict__ words,
    int32_t* __restrict__ first_word, double* __restrict__ score, int32_t* __restrict__ max_common) {
    extern __shared__ double s_kfdb[];
    double* s_val = s_kfdb;                                   // [qcap]
    int32_t* s_id = reinterpret_cast<int32_t*>(s_kfdb + qcap);  // [qcap]
    const int q = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int n = max(min(q_n[q], qcap), 0);
    for (int i = threadIdx.x; i < n; i += PSL_KFDB_WAVES * 64) {
        s_id[i] = q_id[(size_t)q * qstride + i];
        s_val[i] = q_val[(size_t)q * qstride + i];
    }
    __syncthreads();
    const int r0 = blockIdx.x * spb, r1 = min(r0 + spb, nrows);
    for (int r = r0 + wave; r < r1; r += PSL_KFDB_WAVES) {   // wave-uniform
        const int slot = slots ? slots[r] : r;
        const bool on = slot >= 0 && slot < max_kf && row_live[slot] != 0 && !(exclude && exclude[(size_t)q * max_kf + slot]);
        int count = 0, first = -1;
        double sum = 0.0;
        if (on) {
            const int len = min(row_len[slot], row_stride);
            const int32_t* rid = row_id + (size_t)slot * row_stride;
            const double* rval = row_val + (size_t)slot * row_stride;
            for (int base = 0; base < len; base += 64) {
                const int i = base + lane;
                int id = -1;
                bool hit = false;
                double term = 0.0;
                if (i < len) {
                    id = rid[i];
                    int lo = 0, hi = n;   // lower_bound of id among the query's ids
                    while (lo < hi) {
                        const int mid = (lo + hi) >> 1;
                        if (s_id[mid] < id) lo = mid + 1; else hi = mid;
                    }
                    hit = lo < n && s_id[lo] == id;
                    if (hit) {
                        const double vi = s_val[lo], wi = rval[i];   // score(query, keyframe): vi from the query
                        term = fabs(vi - wi) - fabs(vi) - fabs(wi);
                    }
                }
                unsigned long long mask = __ballot(hit);
                if (mask == 0) continue;
                if (first < 0) first = __shfl(id, __ffsll(mask) - 1);
                count += __popcll(mask);
                while (mask) {   // "score += ..." in ascending word order
                    sum += __shfl(term, __ffsll(mask) - 1);
                    mask &= mask - 1;
                }
            }
        }
        if (lane == 0) {
            const size_t o = (size_t)q * nrows + r;
            if (words) words[o] = count;
            if (first_word) first_word[o] = first;
            score[o] = count ? -sum / 2.0 : 0.0;
            if (max_common && count > 0) atomicMax(max_common + q, count);
        }
    }
}

// pslfe_kfdb_add_device: frame f of a pslfe_compute_bow_device result becomes the row of slot0 + f
__global__ __launch_bounds__(256) void k_kfdb_add_rows(const int32_t* __restrict__ src_id, const double* __restrict__ src_val, const int32_t* __restrict__ src_n,
                                                       int stride, int slot0, int row_stride, int32_t* __restrict__ row_id, double* __restrict__ row_val,
                                                       int32_t* __restrict__ row_len, int32_t* __restrict__ row_live) {
    const int f = blockIdx.x, slot = slot0 + f;
    const int n = max(min(min(src_n[f], stride), row_stride), 0);
    for (int i = threadIdx.x; i < n; i += 256) {
        row_id[(size_t)slot * row_stride + i] = src_id[(size_t)f * stride + i];
        row_val[(size_t)slot * row_stride + i] = src_val[(size_t)f * stride + i];
    }
    if (threadIdx.x == 0) { row_len[slot] = n; row_live[slot] = 1; }
}

struct pslfe_kfdb {
    pslfe_ctx* ctx = nullptr;
    int max_kf = 0, max_words = 0;
    int32_t* d_id = nullptr;     // [max_kf][max_words] ascending word ids
    double* d_val = nullptr;     // [max_kf][max_words]
    int32_t* d_len = nullptr;    // [max_kf]
    int32_t* d_live = nullptr;   // [max_kf]
    PslDeviceBuffers mem;        // owns the four
    // host copy of the slot state: what add / erase are checked against, and the order of the adds (the device does not need it)
    std::vector<uint8_t> live;
    std::vector<int64_t> seq;
    int64_t next_seq = 0;
};

static int kfdb_launch(pslfe_kfdb* db, int nrows, const int32_t* d_slots, const int32_t* d_qid, const double* d_qval, const int32_t* d_qn, int nq,
                       int qstride, const uint8_t* d_exclude, int32_t* d_words, int32_t* d_first, double* d_score, int32_t* d_maxc) {
    hipStream_t st = db->ctx->stream;
    if (d_maxc) PSL_HIP(hipMemsetAsync(d_maxc, 0, (size_t)nq * sizeof(int32_t), st));
    if (nrows == 0) return PSLFE_OK;
    // about two workgroups per CU when the launch is large enough for that; a workgroup's staging of the query is shared by its rows
    const long long target = (long long)std::max(db->ctx->cu_count, 1) * 2;
    long long spb = ((long long)nrows * nq + target - 1) / target;
    spb = (spb + PSL_KFDB_WAVES - 1) / PSL_KFDB_WAVES * PSL_KFDB_WAVES;
    spb = std::min<long long>(std::max<long long>(spb, PSL_KFDB_WAVES), PSL_KFDB_MAX_SPB);
    const int qcap = std::min(qstride, PSL_BOW_NMAX);
    PSL_STAGE_BEGIN(db->ctx, "kfdb.query");
    k_kfdb_query<<<dim3((unsigned)((nrows + spb - 1) / spb), (unsigned)nq), PSL_KFDB_WAVES * 64, (size_t)qcap * 12, st>>>(
        db->d_id, db->d_val, db->d_len, db->d_live, db->max_words, db->max_kf, nrows, d_slots, d_qid, d_qval, d_qn, qstride, qcap, d_exclude, (int)spb,
        d_words, d_first, d_score, d_maxc);
    PSL_STAGE_END(db->ctx, "kfdb.query");
    PSL_HIP(hipGetLastError());
    return PSLFE_OK;
}

// a BowVector on the host: ascending non-negative word ids
static int kfdb_check_bow(const char* who, const int32_t* bow_id, const double* bow_val, int n, int max_words) {
    PSL_REQUIRE(n >= 0 && n <= max_words, PSLFE_E_INVALID, "%s: %d words (max_words = %d)", who, n, max_words);
    PSL_REQUIRE(n == 0 || (bow_id && bow_val), PSLFE_E_INVALID, "%s: NULL argument", who);
    for (int i = 0; i < n; ++i)
        PSL_REQUIRE(bow_id[i] >= 0 && (i == 0 || bow_id[i - 1] < bow_id[i]), PSLFE_E_INVALID, "%s: word ids must be ascending (entry %d = %d)", who, i,
                    bow_id[i]);
    return PSLFE_OK;
}

extern "C" {

void pslfe_kfdb_destroy(pslfe_kfdb* db) {
    if (!db) return;
    (void)hipSetDevice(db->ctx->device);
    (void)hipStreamSynchronize(db->ctx->stream);
    delete db;   // its buffers go with it
}

int pslfe_kfdb_create(pslfe_ctx* ctx, int max_keyframes, int max_words, pslfe_kfdb** out) {
    PSL_REQUIRE(ctx && out, PSLFE_E_INVALID, "pslfe_kfdb_create: NULL argument");
    *out = nullptr;
    PSL_REQUIRE(max_keyframes >= 1 && max_keyframes <= (1 << 24) && max_words >= 1 && max_words <= PSL_BOW_NMAX, PSLFE_E_INVALID,
                "pslfe_kfdb_create: %d keyframes (1 .. %d), %d words per keyframe (1 .. %d)", max_keyframes, 1 << 24, max_words, PSL_BOW_NMAX);
    PSL_HIP(hipSetDevice(ctx->device));
    pslfe_kfdb* db = new pslfe_kfdb();
    db->ctx = ctx; db->max_kf = max_keyframes; db->max_words = max_words;
    db->live.assign(max_keyframes, 0);
    db->seq.assign(max_keyframes, -1);
    const size_t rows = (size_t)max_keyframes * max_words;
    db->mem.alloc(db->d_id, rows, "word ids");
    db->mem.alloc(db->d_val, rows, "word values");
    db->mem.alloc(db->d_len, max_keyframes, "row lengths");
    db->mem.alloc(db->d_live, max_keyframes, "live flags");
    int rc = db->mem.check("pslfe_kfdb_create");
    if (!rc) {
        hipError_t e = hipMemsetAsync(db->d_len, 0, (size_t)max_keyframes * 4, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(db->d_live, 0, (size_t)max_keyframes * 4, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) { pslfe_set_error("pslfe_kfdb_create: %s", hipGetErrorString(e)); rc = PSLFE_E_HIP; }
    }
    if (rc) { pslfe_kfdb_destroy(db); return rc; }
    *out = db;
    return PSLFE_OK;
}

int pslfe_kfdb_add(pslfe_kfdb* db, int slot, const int32_t* bow_id, const double* bow_val, int n) {
    PSL_REQUIRE(db, PSLFE_E_INVALID, "pslfe_kfdb_add: NULL argument");
    PSL_REQUIRE(slot >= 0 && slot < db->max_kf, PSLFE_E_INVALID, "pslfe_kfdb_add: slot %d of %d", slot, db->max_kf);
    PSL_REQUIRE(!db->live[slot], PSLFE_E_INVALID, "pslfe_kfdb_add: slot %d is live (erase it first)", slot);
    { const int rc_ = kfdb_check_bow("pslfe_kfdb_add", bow_id, bow_val, n, db->max_words); if (rc_) return rc_; }
    PSL_HIP(hipSetDevice(db->ctx->device));
    hipStream_t st = db->ctx->stream;
    const int32_t one = 1, len = n;
    if (n) {
        PSL_HIP(hipMemcpyAsync(db->d_id + (size_t)slot * db->max_words, bow_id, (size_t)n * 4, hipMemcpyHostToDevice, st));
        PSL_HIP(hipMemcpyAsync(db->d_val + (size_t)slot * db->max_words, bow_val, (size_t)n * 8, hipMemcpyHostToDevice, st));
    }
    PSL_HIP(hipMemcpyAsync(db->d_len + slot, &len, 4, hipMemcpyHostToDevice, st));
    PSL_HIP(hipMemcpyAsync(db->d_live + slot, &one, 4, hipMemcpyHostToDevice, st));
    PSL_HIP(hipStreamSynchronize(st));   // the caller's arrays and the two locals are free again
    db->live[slot] = 1;
    db->seq[slot] = db->next_seq++;
    return PSLFE_OK;
}

int pslfe_kfdb_add_device(pslfe_kfdb* db, int slot0, const int32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow, int nframes, int stride) {
    PSL_REQUIRE(db && d_bow_id && d_bow_val && d_nbow, PSLFE_E_INVALID, "pslfe_kfdb_add_device: NULL argument");
    PSL_REQUIRE(nframes >= 1 && slot0 >= 0 && nframes <= db->max_kf && slot0 <= db->max_kf - nframes, PSLFE_E_INVALID,
                "pslfe_kfdb_add_device: slots %d .. %d of %d", slot0, slot0 + nframes - 1, db->max_kf);
    PSL_REQUIRE(stride >= 1 && stride <= db->max_words, PSLFE_E_INVALID,
                "pslfe_kfdb_add_device: stride %d: a frame's row must fit max_words = %d whatever its count", stride, db->max_words);
    for (int f = 0; f < nframes; ++f)
        PSL_REQUIRE(!db->live[slot0 + f], PSLFE_E_INVALID, "pslfe_kfdb_add_device: slot %d is live (erase it first)", slot0 + f);
    PSL_HIP(hipSetDevice(db->ctx->device));
    k_kfdb_add_rows<<<nframes, 256, 0, db->ctx->stream>>>(d_bow_id, d_bow_val, d_nbow, stride, slot0, db->max_words, db->d_id, db->d_val, db->d_len,
                                                          db->d_live);
    PSL_HIP(hipGetLastError());
    for (int f = 0; f < nframes; ++f) { db->live[slot0 + f] = 1; db->seq[slot0 + f] = db->next_seq++; }
    return PSLFE_OK;
}

int pslfe_kfdb_erase(pslfe_kfdb* db, int slot) {
    PSL_REQUIRE(db, PSLFE_E_INVALID, "pslfe_kfdb_erase: NULL argument");
    PSL_REQUIRE(slot >= 0 && slot < db->max_kf, PSLFE_E_INVALID, "pslfe_kfdb_erase: slot %d of %d", slot, db->max_kf);
    if (!db->live[slot]) return PSLFE_OK;   // KeyFrameDatabase::erase of a keyframe that is not in the lists changes nothing
    PSL_HIP(hipSetDevice(db->ctx->device));
    PSL_HIP(hipMemsetAsync(db->d_live + slot, 0, 4, db->ctx->stream));
    db->live[slot] = 0;
    db->seq[slot] = -1;
    return PSLFE_OK;
}

int pslfe_kfdb_clear(pslfe_kfdb* db) {
    PSL_REQUIRE(db, PSLFE_E_INVALID, "pslfe_kfdb_clear: NULL argument");
    PSL_HIP(hipSetDevice(db->ctx->device));
    PSL_HIP(hipMemsetAsync(db->d_live, 0, (size_t)db->max_kf * 4, db->ctx->stream));
    db->live.assign(db->max_kf, 0);
    db->seq.assign(db->max_kf, -1);
    return PSLFE_OK;
}

int pslfe_kfdb_state(const pslfe_kfdb* db, uint8_t* live, int64_t* seq) {
    PSL_REQUIRE(db, PSLFE_E_INVALID, "pslfe_kfdb_state: NULL argument");
    if (live) memcpy(live, db->live.data(), db->live.size());
    if (seq) memcpy(seq, db->seq.data(), db->seq.size() * sizeof(int64_t));
    return PSLFE_OK;
}

int pslfe_kfdb_query_device(pslfe_kfdb* db, const int32_t* d_bow_id, const double* d_bow_val, const int32_t* d_nbow, int nq, int stride,
                            const uint8_t* d_exclude, int32_t* d_words, int32_t* d_first_word, double* d_score, int32_t* d_max_common) {
    PSL_REQUIRE(db && d_bow_id && d_bow_val && d_nbow && d_words && d_first_word && d_score && d_max_common, PSLFE_E_INVALID,
                "pslfe_kfdb_query_device: NULL argument");
    PSL_REQUIRE(nq >= 1 && nq <= 65535 && stride >= 1 && stride <= PSL_BOW_NMAX, PSLFE_E_INVALID,
                "pslfe_kfdb_query_device: %d queries (1 .. 65535), stride %d (1 .. %d)", nq, stride, PSL_BOW_NMAX);
    PSL_HIP(hipSetDevice(db->ctx->device));
    return kfdb_launch(db, db->max_kf, nullptr, d_bow_id, d_bow_val, d_nbow, nq, stride, d_exclude, d_words, d_first_word, d_score, d_max_common);
}

int pslfe_kfdb_query(pslfe_kfdb* db, const int32_t* bow_id, const double* bow_val, int n, const uint8_t* exclude, int32_t* words, int32_t* first_word,
                     double* score, int* max_common) {
    PSL_REQUIRE(db && words && first_word && score && max_common, PSLFE_E_INVALID, "pslfe_kfdb_query: NULL argument");
    { const int rc_ = kfdb_check_bow("pslfe_kfdb_query", bow_id, bow_val, n, db->max_words); if (rc_) return rc_; }
    const size_t K = (size_t)db->max_kf;
    *max_common = 0;
    if (n == 0) {   // no word, no keyframe reached
        for (size_t s = 0; s < K; ++s) { words[s] = 0; first_word[s] = -1; score[s] = 0.0; }
        return PSLFE_OK;
    }
    PSL_HIP(hipSetDevice(db->ctx->device));
    hipStream_t st = db->ctx->stream;
    { const int rc_ = psl_scratch_begin(db->ctx); if (rc_) return rc_; }
    hipError_t e = hipSuccess;
    const int32_t n32 = n;
    double* d_qval = psl_scratch_up(db->ctx, bow_val, (size_t)n, st, &e);
    int32_t* d_qid = psl_scratch_up(db->ctx, bow_id, (size_t)n, st, &e);
    int32_t* d_qn = psl_scratch_up(db->ctx, &n32, 1, st, &e);
    uint8_t* d_ex = exclude ? psl_scratch_up(db->ctx, exclude, K, st, &e) : nullptr;
    double* d_score = psl_scratch_up<double>(db->ctx, nullptr, K, st, &e);
    int32_t* d_words = psl_scratch_up<int32_t>(db->ctx, nullptr, K, st, &e);
    int32_t* d_first = psl_scratch_up<int32_t>(db->ctx, nullptr, K, st, &e);
    int32_t* d_maxc = psl_scratch_up<int32_t>(db->ctx, nullptr, 1, st, &e);
    int rc = PSLFE_OK;
    if (e == hipSuccess) rc = kfdb_launch(db, db->max_kf, nullptr, d_qid, d_qval, d_qn, 1, n, d_ex, d_words, d_first, d_score, d_maxc);
    int32_t maxc = 0;
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(words, d_words, K * 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(first_word, d_first, K * 4, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(score, d_score, K * 8, hipMemcpyDeviceToHost, st);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(&maxc, d_maxc, 4, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);   // also after a failure: the uploads read the caller's arrays
    if (e == hipSuccess) e = es;
    if (!rc && e != hipSuccess) { pslfe_set_error("pslfe_kfdb_query: %s", hipGetErrorString(e)); rc = PSLFE_E_HIP; }
    if (!rc) *max_common = maxc;
    return rc;
}

int pslfe_kfdb_score(pslfe_kfdb* db, const int32_t* bow_id, const double* bow_val, int n, const int32_t* slots, int nslots, double* score) {
    PSL_REQUIRE(db && nslots >= 0 && (nslots == 0 || (slots && score)), PSLFE_E_INVALID, "pslfe_kfdb_score: NULL argument or %d slots", nslots);
    { const int rc_ = kfdb_check_bow("pslfe_kfdb_score", bow_id, bow_val, n, db->max_words); if (rc_) return rc_; }
    for (int j = 0; j < nslots; ++j) {
        PSL_REQUIRE(slots[j] >= 0 && slots[j] < db->max_kf, PSLFE_E_INVALID, "pslfe_kfdb_score: slot %d of %d", slots[j], db->max_kf);
        PSL_REQUIRE(db->live[slots[j]], PSLFE_E_INVALID, "pslfe_kfdb_score: slot %d is not in the database", slots[j]);
    }
    if (nslots == 0) return PSLFE_OK;
    if (n == 0) {
        for (int j = 0; j < nslots; ++j) score[j] = 0.0;
        return PSLFE_OK;
    }
    PSL_HIP(hipSetDevice(db->ctx->device));
    hipStream_t st = db->ctx->stream;
    { const int rc_ = psl_scratch_begin(db->ctx); if (rc_) return rc_; }
    hipError_t e = hipSuccess;
    const int32_t n32 = n;
    double* d_qval = psl_scratch_up(db->ctx, bow_val, (size_t)n, st, &e);
    int32_t* d_qid = psl_scratch_up(db->ctx, bow_id, (size_t)n, st, &e);
    int32_t* d_qn = psl_scratch_up(db->ctx, &n32, 1, st, &e);
    int32_t* d_slots = psl_scratch_up(db->ctx, slots, (size_t)nslots, st, &e);
    double* d_score = psl_scratch_up<double>(db->ctx, nullptr, (size_t)nslots, st, &e);
    int rc = PSLFE_OK;
    if (e == hipSuccess) rc = kfdb_launch(db, nslots, d_slots, d_qid, d_qval, d_qn, 1, n, nullptr, nullptr, nullptr, d_score, nullptr);
    if (!rc && e == hipSuccess) e = hipMemcpyAsync(score, d_score, (size_t)nslots * 8, hipMemcpyDeviceToHost, st);
    const hipError_t es = hipStreamSynchronize(st);
    if (e == hipSuccess) e = es;
    if (!rc && e != hipSuccess) { pslfe_set_error("pslfe_kfdb_score: %s", hipGetErrorString(e)); rc = PSLFE_E_HIP; }
    return rc;
}

}  // extern "C"
