// ORACLE-internal helpers (test infrastructure only): the pieces more than one oracle source states the same way, statement for
// statement.  Included by the oracle's .cpp files only; nothing here is exported.
#ifndef PSL_ORACLE_INTERNAL_H
#define PSL_ORACLE_INTERNAL_H
#include <stdint.h>

#include <vector>

namespace pso {

// ORBmatcher::DescriptorDistance, src/ORBmatcher.cc:1647-1663 (SWAR popcount of 256 bits)
inline int descriptor_distance(const uint8_t* a, const uint8_t* b) {
    const int32_t* pa = (const int32_t*)a;
    const int32_t* pb = (const int32_t*)b;
    int dist = 0;
    for (int i = 0; i < 8; i++, pa++, pb++) {
        unsigned int v = *pa ^ *pb;
        v = v - ((v >> 1) & 0x55555555);
        v = (v & 0x33333333) + ((v >> 2) & 0x33333333);
        dist += (((v + (v >> 4)) & 0xF0F0F0F) * 0x1010101) >> 24;
    }
    return dist;
}

inline int bin_size(int n) { return n; }
inline int bin_size(const std::vector<int>& v) { return (int)v.size(); }

// ORBmatcher::ComputeThreeMaxima, src/ORBmatcher.cc:1601-1645, on bins given as counts or as lists; the caller sets ind1..3 = -1
template <class Bin>
void three_maxima(const Bin* histo, int L, int& ind1, int& ind2, int& ind3) {
    int max1 = 0, max2 = 0, max3 = 0;
    for (int i = 0; i < L; i++) {
        const int s = bin_size(histo[i]);
        if (s > max1) { max3 = max2; max2 = max1; max1 = s; ind3 = ind2; ind2 = ind1; ind1 = i; }
        else if (s > max2) { max3 = max2; max2 = s; ind3 = ind2; ind2 = i; }
        else if (s > max3) { max3 = s; ind3 = i; }
    }
    if (max2 < 0.1f * (float)max1) { ind2 = -1; ind3 = -1; }
    else if (max3 < 0.1f * (float)max1) { ind3 = -1; }
}

// one row of a float 3x3 * 3x1 product plus a translation: a double sum in this order, rounded once (include/pslfe.h)
inline float affine_row(float m0, float m1, float m2, float x0, float x1, float x2, float t) {
    double a = (double)m0 * (double)x0;
    a += (double)m1 * (double)x1;
    a += (double)m2 * (double)x2;
    a += (double)t;
    return (float)a;
}

// cv::Mat(R) * x + t, R row-major
inline void affine(const float* R, const float* x, const float* t, float* out) {
    for (int r = 0; r < 3; ++r) out[r] = affine_row(R[3 * r], R[3 * r + 1], R[3 * r + 2], x[0], x[1], x[2], t[r]);
}

// the camera centre -R.t() * t of a pose (R, t)
inline void centre(const float* R, const float* t, float* c) {
    for (int r = 0; r < 3; ++r) c[r] = -affine_row(R[r], R[3 + r], R[6 + r], t[0], t[1], t[2], 0.f);
}

}  // namespace pso
#endif
