// A C++ consumer of the KeyFrameDatabase seam of psl-slam_amd/host/pslfe.hpp: what LoopClosing::DetectLoop (src/LoopClosing.cc:124-141)
// and Tracking::Relocalization (src/Tracking.cc:2038) ask of the database, without DBoW2.  The file gives the adds and erases, the
// covisibility neighbours and the queries; per query the program runs the minScore loop over the connected keyframes (Score),
// DetectLoopCandidates with that minScore and DetectRelocalizationCandidates, in this order, on one database.
// tests/test_kfdb_gpu.py builds it with g++, runs it as a child process and compares its output with the restatement.
//
// usage: kfdb_main <case.bin>
//   case.bin: int32 max_keyframes, max_words, nops;
//             nops x { int32 kind (0 add, 1 erase), slot, n; int32 id[n]; f64 val[n] }     (n = 0 for an erase)
//             max_keyframes x { int32 k; int32 neighbour[k] }
//             int32 nq; nq x { int32 n; int32 id[n]; f64 val[n]; int32 nc; int32 connected[nc] }
//   stdout:   {"queries": [{"score_bits": [nc x u64], "min_score_bits": u32, "loop": [...], "reloc": [...]}, ...]}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "../../psl-slam_amd/host/pslfe.hpp"

namespace {
template <class T>
bool rd(FILE* f, std::vector<T>& v, int32_t n) {
    if (n < 0) return false;
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == (size_t)n;
}
bool rdi(FILE* f, int32_t& v) { return fread(&v, 4, 1, f) == 1; }

std::string list(const std::vector<int32_t>& v) {
    std::string s = "[";
    for (size_t i = 0; i < v.size(); ++i) s += (i ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s case.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t K = 0, W = 0, nops = 0;
    if (!rdi(f, K) || !rdi(f, W) || !rdi(f, nops) || K < 1 || nops < 0) { fprintf(stderr, "short header\n"); return 2; }
    try {
        pslfe::Context ctx(0);
        pslfe::KeyFrameDatabase db(ctx, K, W);
        std::vector<int32_t> id;
        std::vector<double> val;
        for (int o = 0; o < nops; ++o) {
            int32_t kind = 0, slot = 0, n = 0;
            if (!rdi(f, kind) || !rdi(f, slot) || !rdi(f, n) || !rd(f, id, n) || !rd(f, val, n)) { fprintf(stderr, "short operation %d\n", o); return 2; }
            if (kind == 0) db.add(slot, id, val); else db.erase(slot);
        }
        std::vector<std::vector<int32_t>> neighbours(K);
        for (int s = 0; s < K; ++s) {
            int32_t k = 0;
            if (!rdi(f, k) || !rd(f, neighbours[s], k)) { fprintf(stderr, "short neighbour list %d\n", s); return 2; }
        }
        int32_t nq = 0;
        if (!rdi(f, nq) || nq < 0) { fprintf(stderr, "short query count\n"); return 2; }
        std::string out = "{\"queries\": [";
        for (int q = 0; q < nq; ++q) {
            int32_t n = 0, nc = 0;
            std::vector<int32_t> connected;
            if (!rdi(f, n) || !rd(f, id, n) || !rd(f, val, n) || !rdi(f, nc) || !rd(f, connected, nc)) { fprintf(stderr, "short query %d\n", q); return 2; }
            const std::vector<double> sc = db.Score(id, val, connected);
            float minScore = 1;
            for (double s : sc) {
                const float score = (float)s;
                if (score < minScore) minScore = score;
            }
            const std::vector<int32_t> loop = db.DetectLoopCandidates(id, val, connected, minScore, neighbours);
            const std::vector<int32_t> reloc = db.DetectRelocalizationCandidates(id, val, neighbours);
            out += std::string(q ? ", " : "") + "{\"score_bits\": [";
            for (size_t i = 0; i < sc.size(); ++i) {
                uint64_t b;
                memcpy(&b, &sc[i], 8);
                out += (i ? ", " : "") + std::to_string(b);
            }
            uint32_t mb;
            memcpy(&mb, &minScore, 4);
            out += "], \"min_score_bits\": " + std::to_string(mb) + ", \"loop\": " + list(loop) + ", \"reloc\": " + list(reloc) + "}";
        }
        fclose(f);
        printf("%s]}\n", out.c_str());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
