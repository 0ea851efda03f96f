// A C++ consumer of the LoopClosing seam of psl-slam_amd/host/pslfe.hpp: the matcher sequence of LoopClosing::ComputeSim3
// (src/LoopClosing.cc:245-400) without OpenCV, DBoW2 or the Sim3 solver.  The current keyframe is matched against every loop
// candidate with ORBmatcher(0.75, true).SearchByBoW (:262-265) in ONE call; the candidate with the most matches stands in for the
// one whose Sim3 was accepted (:296-330), and the loop map points are then searched in the current keyframe's image with
// SearchByProjection(mpCurrentKF, mScw, mvpLoopMapPoints, mvpCurrentMatchedPoints, 10) (:375), the projections given by the file.
// tests/test_loop_match_gpu.py builds it with g++, runs it as a child process and compares its output with the restatement.
//
// usage: loop_main <loop.bin>
//   loop.bin: int32 C; float bounds[4];
//             current keyframe: int32 n1; PslKeyPoint kps[n1]; u8 desc[n1][32]; int32 node[n1]; u8 good[n1] (has a map point, not bad);
//             C x candidate:    int32 n;  PslKeyPoint kps[n];  u8 desc[n][32];  int32 node[n];  u8 good[n];
//             C x projection:   int32 np; PslProjQuery q[np]; u8 qdesc[np][32]; u8 taken[n1]
//   stdout:   {"nmatches": [C], "match": [[per query] x C], "best": c, "proj_nmatches": m, "proj_match": [np], "assigned": [n1]}
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "../../psl-slam_amd/host/pslfe.hpp"

namespace {
struct KF {
    std::vector<PslKeyPoint> kps;
    std::vector<uint8_t> desc, good;
    std::vector<int32_t> node;
    std::map<int32_t, std::vector<int32_t>> featVec;   // DBoW2::FeatureVector: node id -> feature indices, ascending
};

template <class T>
bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}

bool readKF(FILE* f, KF& k) {
    int32_t n = 0;
    if (fread(&n, 4, 1, f) != 1 || n < 0) return false;
    if (!rd(f, k.kps, n) || !rd(f, k.desc, (size_t)n * 32) || !rd(f, k.node, n) || !rd(f, k.good, n)) return false;
    for (int i = 0; i < n; ++i) k.featVec[k.node[i]].push_back(i);
    return true;
}

std::string list(const std::vector<int32_t>& v, size_t a, size_t b) {
    std::string s = "[";
    for (size_t i = a; i < b; ++i) s += (i > a ? ", " : "") + std::to_string(v[i]);
    return s + "]";
}
}  // namespace

int main(int argc, char** argv) {
    if (argc != 2) { fprintf(stderr, "usage: %s loop.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t C = 0;
    float bounds[4];
    if (fread(&C, 4, 1, f) != 1 || fread(bounds, 4, 4, f) != 4 || C < 1) { fprintf(stderr, "short header\n"); return 2; }
    KF cur;
    std::vector<KF> cand(C);
    if (!readKF(f, cur)) { fprintf(stderr, "short current keyframe\n"); return 2; }
    for (int c = 0; c < C; ++c)
        if (!readKF(f, cand[c])) { fprintf(stderr, "short candidate %d\n", c); return 2; }
    std::vector<std::vector<PslProjQuery>> pq(C);
    std::vector<std::vector<uint8_t>> pqdesc(C), taken(C);
    for (int c = 0; c < C; ++c) {
        int32_t np = 0;
        if (fread(&np, 4, 1, f) != 1 || np < 0 || !rd(f, pq[c], np) || !rd(f, pqdesc[c], (size_t)np * 32) || !rd(f, taken[c], cur.kps.size())) {
            fprintf(stderr, "short projection %d\n", c);
            return 2;
        }
    }
    fclose(f);
    try {
        pslfe::Context ctx(0);
        int cap = (int)cur.kps.size();
        for (const KF& k : cand) cap = std::max(cap, (int)k.kps.size());
        pslfe::FrameGrid grid(ctx, std::max(cap, 1), C + 1);   // slots 0..C-1: the candidates, slot C: the current keyframe
        for (int c = 0; c < C; ++c) grid.set(c, cand[c].kps, cand[c].desc, nullptr, bounds[0], bounds[1], bounds[2], bounds[3]);
        grid.set(C, cur.kps, cur.desc, nullptr, bounds[0], bounds[1], bounds[2], bounds[3]);
        // flatten: per candidate its FeatureVector without the features that have no good map point, and one query per feature
        // of the current keyframe with a good map point under every node the two vectors share
        std::vector<int32_t> slots, fidx, fidxOff(1, 0), qOff(1, 0), idx1;
        std::vector<PslBowQuery> q;
        std::vector<uint8_t> qdesc;
        for (int c = 0; c < C; ++c) {
            slots.push_back(c);
            std::map<int32_t, std::pair<int32_t, int32_t>> run;
            const int32_t f0 = fidxOff.back();
            for (const auto& nd : cand[c].featVec) {
                const int32_t start = (int32_t)fidx.size() - f0;
                for (int32_t i : nd.second)
                    if (cand[c].good[i]) fidx.push_back(i);
                run[nd.first] = std::make_pair(start, (int32_t)fidx.size() - f0 - start);
            }
            fidxOff.push_back((int32_t)fidx.size());
            for (const auto& nd : cur.featVec) {
                const auto r = run.find(nd.first);
                if (r == run.end()) continue;
                for (int32_t i : nd.second) {
                    if (!cur.good[i]) continue;
                    q.push_back(PslBowQuery{r->second.first, r->second.second, cur.kps[i].angle});
                    qdesc.insert(qdesc.end(), cur.desc.begin() + (size_t)i * 32, cur.desc.begin() + (size_t)i * 32 + 32);
                    idx1.push_back(i);
                }
            }
            qOff.push_back((int32_t)q.size());
        }
        pslfe::KeyFrameMatcher matcher(ctx);
        std::vector<int32_t> match, nmatches, pmatch, assigned;
        matcher.SearchByBoWCandidates(grid, slots, fidx, fidxOff, q, qdesc, qOff, match, nmatches, 0.75f, true);
        const int best = (int)(std::max_element(nmatches.begin(), nmatches.end()) - nmatches.begin());
        const int pn = matcher.SearchByProjectionSim3(grid, C, pq[best], pqdesc[best], taken[best], pmatch, assigned);
        std::string s = "{\"nmatches\": " + list(nmatches, 0, nmatches.size()) + ", \"match\": [";
        for (int c = 0; c < C; ++c) s += (c ? ", " : "") + list(match, qOff[c], qOff[c + 1]);
        s += "], \"best\": " + std::to_string(best) + ", \"proj_nmatches\": " + std::to_string(pn);
        s += ", \"proj_match\": " + list(pmatch, 0, pmatch.size()) + ", \"assigned\": " + list(assigned, 0, assigned.size()) + "}";
        printf("%s\n", s.c_str());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
