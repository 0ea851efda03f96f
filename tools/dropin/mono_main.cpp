// A C++ consumer of the monocular seam of psl-slam_amd/host/pslfe.hpp: Tracking::GrabImageMonocular (src/Tracking.cc:245-291) with
// the initialiser's extractor (2 x nFeatures, src/Tracking.cc:132, :265) and the matching part of Tracking::MonocularInitialization
// (src/Tracking.cc:659-704): the first frame with more than 100 keypoints becomes the initial frame (vbPrevMatched = its mvKeysUn),
// every later frame is matched against it with ORBmatcher(0.9, true).SearchForInitialization(..., 100), prev chained across calls,
// and the initial frame is dropped when a frame has <= 100 keypoints or fewer than 100 matches.  Initializer (the geometric
// solver) is out of scope.  tests/test_mono_init_gpu.py builds it with g++, runs it as a child process and compares its output
// with the Python path.
//
// usage: mono_main <seq.bin> <nfeatures>
//   seq.bin: int32 w, h, nframes; float fx fy cx cy k1 k2 p1 p2 k3 bf; u8 frames[nframes][h][w]
//   stdout:  {"keypoints": [...], "matches": [...]} with matches[t] = nmatches of frame t, -1 where no search ran
#include <stdio.h>
#include <stdlib.h>

#include <string>
#include <vector>

#include "../../psl-slam_amd/host/pslfe.hpp"

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s seq.bin nfeatures\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
    int hdr[3];
    PslCamera cam;
    if (fread(hdr, sizeof(int), 3, f) != 3 || fread(&cam, sizeof(cam), 1, f) != 1) { fprintf(stderr, "short header\n"); return 2; }
    const int w = hdr[0], h = hdr[1], nframes = hdr[2];
    std::vector<uint8_t> frames((size_t)w * h * nframes);
    if (fread(frames.data(), 1, frames.size(), f) != frames.size()) { fprintf(stderr, "short frames\n"); return 2; }
    fclose(f);
    std::vector<int> nkps, nmatches;
    try {
        pslfe::Context ctx(0);
        const int nfeatures = atoi(argv[2]);
        pslfe::ORBextractor ini(ctx, 2 * nfeatures, 1.2f, 8, 20, 7);   // mpIniORBextractor
        const int cap = std::max(pslfe_orb_max_keypoints(ini.get(), w, h), 1);
        pslfe::FrameGrid grid(ctx, cap, 2);                            // slot 0: mInitialFrame, slot 1: mCurrentFrame
        pslfe::ORBmatcher matcher(0.9f, true);
        bool initializing = false;                                     // mpInitializer != NULL
        std::vector<float> prev;                                       // mvbPrevMatched
        std::vector<int32_t> iniMatches;                               // mvIniMatches
        std::vector<PslKeyPoint> kps, un;
        std::vector<uint8_t> desc;
        std::vector<float> depth, uright;
        for (int t = 0; t < nframes; ++t) {
            ini(frames.data() + (size_t)t * w * h, w, h, w, kps, desc);
            const int n = (int)kps.size();
            nkps.push_back(n);
            int nm = -1;
            if (!initializing) {
                if (n > 100) {
                    grid.setMono(0, ini, 0, 1, cam);
                    grid.fetch(0, un, depth, uright, cap);
                    prev.resize(2 * un.size());
                    for (size_t i = 0; i < un.size(); ++i) { prev[2 * i] = un[i].x; prev[2 * i + 1] = un[i].y; }
                    initializing = true;
                }
            } else if (n <= 100) {
                initializing = false;
            } else {
                grid.setMono(1, ini, 0, 1, cam);
                nm = matcher.SearchForInitialization(grid, 0, grid, 1, prev, iniMatches, 100);
                if (nm < 100) initializing = false;
            }
            nmatches.push_back(nm);
        }
    } catch (const std::exception& e) {
        fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::string s = "{\"keypoints\": [";
    for (size_t t = 0; t < nkps.size(); ++t) s += (t ? ", " : "") + std::to_string(nkps[t]);
    s += "], \"matches\": [";
    for (size_t t = 0; t < nmatches.size(); ++t) s += (t ? ", " : "") + std::to_string(nmatches[t]);
    s += "]}";
    printf("%s\n", s.c_str());
    return 0;
}
