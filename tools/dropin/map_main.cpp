// A C++ consumer of the map-upkeep seam of psl-slam_amd/host/pslfe.hpp: the tail of LocalMapping::ProcessNewKeyFrame
// (src/LocalMapping.cc:150-190: ComputeDistinctiveDescriptors and UpdateNormalAndDepth for the map points the new keyframe sees)
// followed by the point half of SearchInNeighbors (:790-797: Fuse into every neighbour) and the ComputeSceneMedianDepth of the
// neighbours (:324), without OpenCV.  The file gives a seeded map: keyframes, map point positions, their observations.  The refreshed
// rows are not looked at by the program: they go straight into FuseKeyFrames, as a caller would pass them on.
// tests/test_map_upkeep_gpu.py builds it with g++, runs it as a child process and compares its dump with the restatement.
//
// usage: map_main <map.bin> <out.bin>
//   map.bin: int32 S, K, M, nkf, nlevels, q; float bounds[4]; PslCamera cam; float scale[nlevels], inv_sigma2[nlevels], log_scale, th;
//            S x keyframe of the store: int32 n; PslKeyPoint kps[n]; u8 desc[n][32]; float uright[n];
//            PslKfView views[K];                                        the neighbours: pose and slot
//            PslMapPointGeom mp[M];                                     positions; the rest is whatever the map held before
//            int32 obs_off[M+1], obs_kf[nobs]; u8 obs_desc[nobs][32];   mObservations in iteration order, the observed descriptors
//            float centres[nkf][3]; int32 ref_kf[M], ref_level[M]; u8 bad[M];
//            u8 fuse_skip[K][M];                                        isBad / IsInKeyFrame of SearchInNeighbors
//            int32 med_off[K+1]; float med_x[med_off[K]][3]             the map points of every neighbour
//   out.bin: int32 best[M]; PslMapPointGeom mp[M]; int32 bestIdx[K*M], bestDist[K*M]; PslProjQuery rows[K*M]; float depth[K]
//   stdout:  {"points": M, "refreshed": r, "fused": f, "depth": [K floats]}
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../psl-slam_amd/host/pslfe.hpp"

namespace {
template <class T>
bool rd(FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
template <class T>
bool wr(FILE* f, const std::vector<T>& v) { return v.empty() || fwrite(v.data(), sizeof(T), v.size(), f) == v.size(); }

struct KF {
    std::vector<PslKeyPoint> kps;
    std::vector<uint8_t> desc;
    std::vector<float> uright;
};
}  // namespace

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s map.bin out.bin\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int32_t hdr[6];
    float bounds[4], tail[2];
    PslCamera cam;
    if (fread(hdr, 4, 6, f) != 6 || fread(bounds, 4, 4, f) != 4 || fread(&cam, sizeof(cam), 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int S = hdr[0], K = hdr[1], M = hdr[2], nkf = hdr[3], nlevels = hdr[4], q = hdr[5];
    if (S < 1 || K < 0 || M < 0 || nkf < 0 || nlevels < 1 || nlevels > PSLFE_MAX_LEVELS) { fprintf(stderr, "bad header\n"); return 2; }
    std::vector<float> scale, invSigma2;
    if (!rd(f, scale, nlevels) || !rd(f, invSigma2, nlevels) || fread(tail, 4, 2, f) != 2) { fprintf(stderr, "short tables\n"); return 2; }
    std::vector<KF> kfs(S);
    for (KF& k : kfs) {
        int32_t n = 0;
        if (fread(&n, 4, 1, f) != 1 || n < 0 || !rd(f, k.kps, n) || !rd(f, k.desc, (size_t)n * 32) || !rd(f, k.uright, n)) {
            fprintf(stderr, "short keyframe\n");
            return 2;
        }
    }
    std::vector<PslKfView> views;
    std::vector<PslMapPointGeom> mp;
    std::vector<int32_t> obsOff, obsKf, refKf, refLevel, medOff;
    std::vector<uint8_t> obsDesc, bad, fuseSkip;
    std::vector<float> centres, medX;
    bool ok = rd(f, views, K) && rd(f, mp, M) && rd(f, obsOff, (size_t)M + 1) && obsOff[M] >= 0;
    ok = ok && rd(f, obsKf, obsOff[M]) && rd(f, obsDesc, (size_t)obsOff[M] * 32) && rd(f, centres, (size_t)nkf * 3);
    ok = ok && rd(f, refKf, M) && rd(f, refLevel, M) && rd(f, bad, M) && rd(f, fuseSkip, (size_t)K * M);
    ok = ok && rd(f, medOff, (size_t)K + 1) && medOff[K] >= 0 && rd(f, medX, (size_t)medOff[K] * 3);
    fclose(f);
    if (!ok) { fprintf(stderr, "short map\n"); return 2; }
    try {
        pslfe::Context ctx(0);
        size_t cap = 1;
        for (const KF& k : kfs) cap = std::max(cap, k.kps.size());
        pslfe::FrameGrid grid(ctx, (int)cap, S);
        for (int s = 0; s < S; ++s) grid.set(s, kfs[s].kps, kfs[s].desc, kfs[s].uright.data(), bounds[0], bounds[1], bounds[2], bounds[3]);
        pslfe::KeyFrameMatcher matcher(ctx);
        // ProcessNewKeyFrame: pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth();
        const std::vector<int32_t> best = matcher.ComputeDistinctiveDescriptors(obsDesc, obsOff);
        std::vector<uint8_t> mpdesc((size_t)M * 32, 0);
        for (int i = 0; i < M; ++i)
            if (best[i] >= 0) memcpy(&mpdesc[(size_t)i * 32], &obsDesc[((size_t)obsOff[i] + best[i]) * 32], 32);
        matcher.UpdateNormalAndDepth(mp, obsOff, obsKf, centres, refKf, refLevel, bad, scale);
        // SearchInNeighbors: matcher.Fuse(pKFi, vpMapPointMatches) for every neighbour, the refreshed rows as they are
        std::vector<int32_t> bestIdx, bestDist;
        std::vector<PslProjQuery> rows;
        matcher.FuseKeyFrames(grid, PSLFE_KF_PROJ_FUSE, views, mp, mpdesc, fuseSkip, cam, bounds, scale, &invSigma2, tail[0], tail[1], bestIdx, bestDist,
                              &rows);
        // CreateNewMapPoints (monocular): pKF2->ComputeSceneMedianDepth(2) per neighbour
        std::vector<PslPose> poses;
        for (const PslKfView& v : views) poses.push_back(v.Tcw);
        const std::vector<float> depth = matcher.ComputeSceneMedianDepth(poses, medX, medOff, q);

        FILE* o = fopen(argv[2], "wb");
        if (!o || !wr(o, best) || !wr(o, mp) || !wr(o, bestIdx) || !wr(o, bestDist) || !wr(o, rows) || !wr(o, depth) || fclose(o) != 0) {
            fprintf(stderr, "cannot write %s\n", argv[2]);
            return 2;
        }
        int refreshed = 0, fused = 0;
        for (int i = 0; i < M; ++i) refreshed += obsOff[i + 1] > obsOff[i] && !bad[i];
        for (int32_t d : bestDist) fused += d <= pslfe::KeyFrameMatcher::TH_LOW;
        std::string s = "{\"points\": " + std::to_string(M) + ", \"refreshed\": " + std::to_string(refreshed) + ", \"fused\": " + std::to_string(fused) +
                        ", \"depth\": [";
        for (size_t k = 0; k < depth.size(); ++k) s += (k ? ", " : "") + std::to_string(depth[k]);
        printf("%s]}\n", s.c_str());
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    return 0;
}
