// Sequential restatement of the monocular initialiser's matcher, in this project's words: the frame grid of the frame store
// (64 x 48 cells, CSR in the order the window search visits them) and SearchForInitialization on it, one query after the
// other.  Test infrastructure for tests/test_mono_init_*.py and tools/bench_mono_init.py, part of the oracle library: built with
// -ffp-contract=off so every float operation is rounded on its own, as on the device.
#include <math.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <climits>
#include <vector>

#include "psl_oracle.h"
#include "psl_oracle_internal.h"

namespace {

constexpr int kCols = 64, kRows = 48, kCells = kCols * kRows, kHisto = 30, kThLow = 50;

struct Grid {
    float minX, minY, invW, invH;
    std::vector<int> start, idx;   // CSR, cell = ix * 48 + iy
};

Grid make_grid(const PsoKeyPoint* k, int n, const float* b) {
    Grid g;
    g.minX = b[0]; g.minY = b[1];
    g.invW = (float)kCols / (b[2] - b[0]);
    g.invH = (float)kRows / (b[3] - b[1]);
    g.start.assign(kCells + 1, 0);
    g.idx.resize(n > 0 ? n : 1);
    g.idx.resize(pso_grid_build(k, n, b[0], b[1], b[2], b[3], g.start.data(), g.idx.data()));
    return g;
}

// the octave-0 keypoints of the window of radius r around (x, y), in visiting order
void window0(const Grid& g, const PsoKeyPoint* k, float x, float y, float r, std::vector<int>& out) {
    out.clear();
    const int x0 = std::max(0, (int)floorf((x - g.minX - r) * g.invW));
    const int x1 = std::min(kCols - 1, (int)ceilf((x - g.minX + r) * g.invW));
    const int y0 = std::max(0, (int)floorf((y - g.minY - r) * g.invH));
    const int y1 = std::min(kRows - 1, (int)ceilf((y - g.minY + r) * g.invH));
    if (x0 >= kCols || x1 < 0 || y0 >= kRows || y1 < 0) return;
    for (int ix = x0; ix <= x1; ++ix)
        for (int iy = y0; iy <= y1; ++iy)
            for (int p = g.start[ix * kRows + iy]; p < g.start[ix * kRows + iy + 1]; ++p) {
                const PsoKeyPoint& c = k[g.idx[p]];
                if (c.octave != 0) continue;
                if (fabsf(c.x - x) < r && fabsf(c.y - y) < r) out.push_back(g.idx[p]);
            }
}
}  // namespace

extern "C" {

// CSR of the grid of n keypoints with bounds {minX, minY, maxX, maxY}: start[64*48+1], idx[n]; returns the entry count
int mr_grid(const PsoKeyPoint* kps, int n, const float* bounds, int32_t* start, int32_t* idx) {
    return pso_grid_build(kps, n, bounds[0], bounds[1], bounds[2], bounds[3], start, idx);
}

// SearchForInitialization.  prev: [n1][2] in/out; m12: [n1] out; accepted: [n1] out or NULL (the keypoint a query accepted,
// also when a later query took it; -1 if it never accepted); returns the match count.
int mr_search(const PsoKeyPoint* k1, const uint8_t* desc1, int n1, const PsoKeyPoint* k2, const uint8_t* desc2, int n2,
              const float* bounds2, float* prev, int window, float nnratio, int check_ori, int32_t* m12, int32_t* accepted) {
    const Grid g = make_grid(k2, n2, bounds2);
    const float r = (float)window;
    std::vector<int> best_of(n2, INT_MAX), owner(n2, -1), took(n1, -1), bin(n1, -1), cand;
    for (int i = 0; i < n1; ++i) m12[i] = -1;
    std::vector<int> hist(kHisto, 0);
    for (int q = 0; q < n1; ++q) {
        if (k1[q].octave != 0) continue;
        window0(g, k2, prev[2 * q], prev[2 * q + 1], r, cand);
        int d1 = INT_MAX, d2 = INT_MAX, pick = -1;
        for (int c : cand) {
            const int d = pso::descriptor_distance(desc1 + 32 * (size_t)q, desc2 + 32 * (size_t)c);
            if (best_of[c] <= d) continue;            // a better match holds c already
            if (d < d1) { d2 = d1; d1 = d; pick = c; }
            else if (d < d2) d2 = d;
        }
        if (!(d1 <= kThLow && (float)d1 < (float)d2 * nnratio)) continue;
        if (owner[pick] >= 0) m12[owner[pick]] = -1;  // the earlier query loses it for good
        m12[q] = pick;
        owner[pick] = q;
        best_of[pick] = d1;
        took[q] = pick;
        if (check_ori) {
            float rot = k1[q].angle - k2[pick].angle;
            if (rot < 0.0f) rot += 360.0f;
            int b = (int)roundf(rot * (1.0f / kHisto));
            if (b == kHisto) b = 0;
            bin[q] = b;
            ++hist[b];                                 // stays, whatever happens to m12[q] later
        }
    }
    if (check_ori) {
        int b1 = -1, b2 = -1, b3 = -1;
        pso::three_maxima(hist.data(), kHisto, b1, b2, b3);
        for (int q = 0; q < n1; ++q)
            if (m12[q] >= 0 && bin[q] != b1 && bin[q] != b2 && bin[q] != b3) m12[q] = -1;
    }
    int n = 0;
    for (int q = 0; q < n1; ++q)
        if (m12[q] >= 0) {
            prev[2 * q] = k2[m12[q]].x;
            prev[2 * q + 1] = k2[m12[q]].y;
            ++n;
        }
    if (accepted) memcpy(accepted, took.data(), sizeof(int) * (size_t)n1);
    return n;
}

}  // extern "C"
