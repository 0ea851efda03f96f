// Initializer (src/Initializer.cc), the two-view map initialisation of Tracking::MonocularInitialization (src/Tracking.cc:659-760), as
// functions of one thread: the draw of eight rows, Normalize, the 8-point homography and fundamental matrix with this library's reading
// of OpenCV's float Jacobi SVD, the two symmetric transfer scores of a row, the motion hypotheses of ReconstructF / ReconstructH,
// CheckRT / Triangulate for one row, the two decision trees, and the driver psl_init_initialize_host in the reference's order.
// Product code.  Plain C++ text: the kernel (pslfe_initializer.hip) includes it for the device and tools/dropin/init_main.cpp for its
// host loop (define PSL_INIT_HOST_ONLY there to build without the library), so both run the same single IEEE operations (build with
// -ffp-contract=off).  tests/initializer_cases.py is the same text in numpy.
// Restated from the reference, rounding by rounding (DESIGN.md §3 lists every convention):
//   the constructor, the head of Initialize      src/Initializer.cc:33-97; Thirdparty/DBoW2/DUtils/Random.cpp:47-50
//   FindHomography, FindFundamental              :124-223
//   ComputeH21, ComputeF21                       :226-303
//   CheckHomography, CheckFundamental            :305-468
//   ReconstructF, ReconstructH                   :470-732
//   Triangulate, Normalize, CheckRT, DecomposeE  :734-929
// glibc's rand(), RandomInt, the draw (psl_rs_draw<8>) and the Jacobi SVD are those of ransac_kernels.h: included, not copied.
// OpenCV is not in the reference tree: every step handed to it is this library's reading of OpenCV 3.2; parity with OpenCV is unpinned.
//   cv::SVD::compute / SVDecomp, CV_32F   psl_init_jacobi, psl_init_complete: psl_rs_jacobi_svd<float> (ransac_kernels.h holds the reading)
//                                on the n rows (length m) of At = A^T with eps = 2 * FLT_EPSILON; with m < n the operands are swapped, so
//                                the 8x9 matrix of ComputeF21 runs on its own 8 rows and vt is the "U" side, 9x9.  Then, with minval =
//                                FLT_MIN, every row i < n1 (n1 = the full size with FULL_UV) is divided by its
//                                singular value; a row with sd <= minval, and every row n..n1-1, is first completed: filled with +-1/m,
//                                the sign from (next() & 256) of RNG(0x12345678) (multiply with carry, state * 4164903690 + (state >>
//                                32)), orthogonalised twice against the earlier rows (dot product in double of the float products,
//                                each pass followed by a division by the float sum of magnitudes when that exceeds 100 eps), normalised.
//                                vt.row(8) of ComputeF21 is exactly such a row.
//   Mat * Mat, 3x3 / 3x4 / 3x1, no transposed operand   the small-matrix branch of gemm: float, left to right, then * alpha (a float
//                                product for the scalar of s*U*Rp) and + the addend (R*p + t) as float operations.
//   Mat * Mat with a transposed operand (K.t()*F21, -R.t()*t, u*W.t())   the generic path: double accumulators from 0.0 over the
//                                widened floats in index order, times alpha in double, rounded to float.
//   Mat::inv() at 3x3            the cofactors in double times 1 / det (det in double), rounded to float; det == 0 gives zeros.
//   cv::determinant at 3x3       in double.
//   cv::norm, Mat::dot           sequential double sums of the widened floats' products; norm takes the sqrt.
//   Mat / scalar                 times 1.0 / scalar in double, rounded to float.
//   x * row - row (Triangulate)  float operations.
// What the reference leaves undefined (include/pslfe.h states the same):
//   fewer than 8 matches         nothing is drawn or solved, status 0 (the reference indexes an empty vector)
//   no model                     neither search has a hypothesis with a score above 0.0 (identical points give sX = inf and NaN scores):
//                                status bit 2, nothing reconstructed (the reference would hand an empty cv::Mat to ReconstructF)
//   a NaN in vCosParallax        the order of psl_init_cos_key: by the bit pattern, a NaN with the sign bit set below -inf, one with it
//                                clear above +inf (std::sort is undefined there)
//   FindFundamental sizes its vectors from the still empty vbMatchesInliers (:178); harmless, CheckFundamental resizes (:404).
// Normalize runs twice in the reference (once per search thread) with identical results; here once.
#ifndef PSL_INITIALIZER_KERNELS_H
#define PSL_INITIALIZER_KERNELS_H

#include "../../include/pslfe.h"
#include <string.h>

#include "ransac_kernels.h"

#ifdef __clang__
#pragma clang fp contract(off)
#endif

// every function is inlined into its caller: a call on the device would put a frame into scratch memory
#define PSL_INIT_HD __attribute__((always_inline)) PSL_PO_HD
#define PSL_INIT_FLT_MIN 1.17549435082228750797e-38
#define PSL_INIT_FSQRT(x) ((float)PSL_PO_SQRT((double)(x)))   // the correctly rounded float root: 53 >= 2 * 24 + 2
#define PSL_INIT_PI 3.1415926535897932384626433832795

#define PSL_ACOSF_HD PSL_INIT_HD
#define PSL_ACOSF_DIV(a, b) PSL_RS_FDIV(a, b)
#define PSL_ACOSF_SQRT(a) PSL_INIT_FSQRT(a)
#include "psl_acosf.h"

// The workspace of one hypothesis: floats A (the rows of At) and V (Vt), doubles W.  Element k lies at a[k * ES]: ES = 1 on the
// host; the kernel interleaves the workspaces of a block of hypotheses (and later of the rows of a chunk).
enum {
    PSL_INIT_WS_A = 0,     // 144: 9 rows of 16 (ComputeH21); 9 rows of 9 (ComputeF21), then 9 more at 81 for the 3x3
    PSL_INIT_WS_V = 144,   // 81
    PSL_INIT_WS_F = 225,
    PSL_INIT_WS_D = 9,     // doubles
    PSL_INIT_RT_F = 32,    // Triangulate: A 16, V 16
    PSL_INIT_RT_D = 4
};
#define F_(p, k) (p)[(size_t)(k) * ES]

struct PslInitNorm {
    float mx, my, sx, sy;   // T = [sx 0 -mx*sx; 0 sy -my*sy; 0 0 1]
};

// Where the matched rows are: the first lds_n in `lds` (stride 5 words: u1 v1 u2 v2 and the frame-1 keypoint), the others read
// through row_i from the keypoints where they are used.  The host keeps lds_n = 0.
struct PslInitRows {
    const float* lds;
    int lds_n;
    const int32_t* row_i;     // [N] mvMatches12[r].first
    const int32_t* matches;   // vMatches12
    const float* k1;
    const float* k2;
    size_t ks;                // keypoint stride in floats
};
PSL_INIT_HD int psl_init_load(const PslInitRows* R, int r, float* q) {
    if (r < R->lds_n) {
        const float* s = R->lds + 5 * (size_t)r;
        q[0] = s[0]; q[1] = s[1]; q[2] = s[2]; q[3] = s[3];
        int i1;
        __builtin_memcpy(&i1, s + 4, 4);
        return i1;
    }
    const int i1 = R->row_i[r], i2 = R->matches[i1];
    q[0] = R->k1[R->ks * (size_t)i1]; q[1] = R->k1[R->ks * (size_t)i1 + 1];
    q[2] = R->k2[R->ks * (size_t)i2]; q[3] = R->k2[R->ks * (size_t)i2 + 1];
    return i1;
}

// ---- Normalize (:749-795), one coordinate of one frame: comp 0 = x, 1 = y.  Sequential float sums in keypoint order ------------------
PSL_INIT_HD void psl_init_normalize(const float* keys, size_t ks, int n, int comp, float* mean, float* scale) {
    float m = 0;
    for (int i = 0; i < n; ++i) m = m + keys[ks * (size_t)i + comp];
    m = PSL_RS_FDIV(m, (float)n);
    float dev = 0;
    for (int i = 0; i < n; ++i) dev = dev + __builtin_fabsf(keys[ks * (size_t)i + comp] - m);
    dev = PSL_RS_FDIV(dev, (float)n);
    *mean = m;
    *scale = (float)PSL_PO_DIV(1.0, (double)dev);
}
PSL_INIT_HD void psl_init_T(const PslInitNorm* n, float* T) {
    T[0] = n->sx; T[1] = 0.f; T[2] = -n->mx * n->sx;
    T[3] = 0.f; T[4] = n->sy; T[5] = -n->my * n->sy;
    T[6] = 0.f; T[7] = 0.f; T[8] = 1.f;
}

// ---- small matrices ----------------------------------------------------------------------------------------------------------------
// gemm's small-matrix branch: float, left to right
PSL_INIT_HD void psl_init_mul33(const float* a, const float* b, float* d) {
    float t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) t[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
    for (int k = 0; k < 9; ++k) d[k] = t[k];
}
PSL_INIT_HD void psl_init_mul31(const float* a, const float* b, float* d) {
    for (int i = 0; i < 3; ++i) d[i] = (a[3 * i] * b[0] + a[3 * i + 1] * b[1]) + a[3 * i + 2] * b[2];
}
// the generic path: d = a^T * b (ta) or a * b^T (tb), double accumulators
PSL_INIT_HD void psl_init_mul33_t(const float* a, const float* b, int ta, float* d) {
    float t[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            double s = 0.0;
            for (int k = 0; k < 3; ++k) s = s + (double)(ta ? a[3 * k + i] : a[3 * i + k]) * (double)(ta ? b[3 * k + j] : b[3 * j + k]);
            t[3 * i + j] = (float)s;
        }
    for (int k = 0; k < 9; ++k) d[k] = t[k];
}
PSL_INIT_HD double psl_init_det3(const float* m) {
    return ((double)m[0] * ((double)m[4] * (double)m[8] - (double)m[5] * (double)m[7]) -
            (double)m[1] * ((double)m[3] * (double)m[8] - (double)m[5] * (double)m[6])) +
           (double)m[2] * ((double)m[3] * (double)m[7] - (double)m[4] * (double)m[6]);
}
PSL_INIT_HD void psl_init_inv3(const float* S, float* D) {
    double d = psl_init_det3(S);
    if (d == 0.0) {
        for (int k = 0; k < 9; ++k) D[k] = 0.f;
        return;
    }
    d = PSL_PO_DIV(1.0, d);
    double t[9];
#define S_(r, c) ((double)S[3 * (r) + (c)])
    t[0] = (S_(1, 1) * S_(2, 2) - S_(1, 2) * S_(2, 1)) * d;
    t[1] = (S_(0, 2) * S_(2, 1) - S_(0, 1) * S_(2, 2)) * d;
    t[2] = (S_(0, 1) * S_(1, 2) - S_(0, 2) * S_(1, 1)) * d;
    t[3] = (S_(1, 2) * S_(2, 0) - S_(1, 0) * S_(2, 2)) * d;
    t[4] = (S_(0, 0) * S_(2, 2) - S_(0, 2) * S_(2, 0)) * d;
    t[5] = (S_(0, 2) * S_(1, 0) - S_(0, 0) * S_(1, 2)) * d;
    t[6] = (S_(1, 0) * S_(2, 1) - S_(1, 1) * S_(2, 0)) * d;
    t[7] = (S_(0, 1) * S_(2, 0) - S_(0, 0) * S_(2, 1)) * d;
    t[8] = (S_(0, 0) * S_(1, 1) - S_(0, 1) * S_(1, 0)) * d;
#undef S_
    for (int k = 0; k < 9; ++k) D[k] = (float)t[k];
}
// v / cv::norm(v)
PSL_INIT_HD void psl_init_unit3(float* v) {
    const double n = PSL_PO_SQRT(((double)v[0] * (double)v[0] + (double)v[1] * (double)v[1]) + (double)v[2] * (double)v[2]);
    const double inv = PSL_PO_DIV(1.0, n);
    for (int k = 0; k < 3; ++k) v[k] = (float)((double)v[k] * inv);
}

// ---- cv::SVD::compute on CV_32F: psl_rs_jacobi_svd<float> with eps = 2 * FLT_EPSILON; the left side is psl_init_complete's ----------
template <int ES>
PSL_INIT_HD void psl_init_jacobi(float* a, int m, int n, double* w, float* v) {
    psl_rs_jacobi_svd<float, ES>(a, m, n, w, v, (double)(PSL_RS_FLT_EPSILON * 2));
}
// The left side: rows 0..n1-1 of a (n1 >= n rows of storage) divided by their singular value, completed where there is none
template <int ES>
PSL_INIT_HD void psl_init_complete(float* a, int m, int n, int n1, const double* w) {
    const double minval = PSL_INIT_FLT_MIN;
    const float eps = PSL_RS_FLT_EPSILON * 2;
    unsigned long long state = 0x12345678ull;
    for (int i = 0; i < n1; ++i) {
        double sd = i < n ? F_(w, i) : 0.0;
        for (int ii = 0; ii < 100 && sd <= minval; ++ii) {
            const float val0 = (float)PSL_PO_DIV(1.0, (double)m);
            for (int k = 0; k < m; ++k) {
                state = (unsigned long long)(unsigned)state * 4164903690ull + (state >> 32);
                F_(a, i * m + k) = ((unsigned)state & 256u) != 0 ? val0 : -val0;
            }
            for (int iter = 0; iter < 2; ++iter)
                for (int j = 0; j < i; ++j) {
                    sd = 0;
                    for (int k = 0; k < m; ++k) sd = sd + (double)(F_(a, i * m + k) * F_(a, j * m + k));
                    float asum = 0;
                    for (int k = 0; k < m; ++k) {
                        const float t = (float)((double)F_(a, i * m + k) - sd * (double)F_(a, j * m + k));
                        F_(a, i * m + k) = t;
                        asum = asum + __builtin_fabsf(t);
                    }
                    asum = asum > eps * 100 ? PSL_RS_FDIV(1.f, asum) : 0.f;
                    for (int k = 0; k < m; ++k) F_(a, i * m + k) = F_(a, i * m + k) * asum;
                }
            sd = 0;
            for (int k = 0; k < m; ++k) { const double t = (double)F_(a, i * m + k); sd = sd + t * t; }
            sd = PSL_PO_SQRT(sd);
        }
        const float s = (float)(sd > minval ? PSL_PO_DIV(1.0, sd) : 0.);
        for (int k = 0; k < m; ++k) F_(a, i * m + k) = F_(a, i * m + k) * s;
    }
}
// cv::SVD::compute of a 3x3 float matrix: u, w, vt.  a: 9 floats, v: 9 floats, w: 3 doubles of workspace
template <int ES>
PSL_INIT_HD void psl_init_svd3(const float* M, float* a, double* w, float* v, float* u, float* wf, float* vt) {
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) F_(a, 3 * i + k) = M[3 * k + i];
    psl_init_jacobi<ES>(a, 3, 3, w, v);
    psl_init_complete<ES>(a, 3, 3, 3, w);
    for (int i = 0; i < 3; ++i) {
        wf[i] = (float)F_(w, i);
        for (int k = 0; k < 3; ++k) { u[3 * k + i] = F_(a, 3 * i + k); vt[3 * i + k] = F_(v, 3 * i + k); }
    }
}

// ---- ComputeH21 (:226-266) + the de-normalisation (:159-161): ws holds PSL_INIT_WS_F floats, wd PSL_INIT_WS_D doubles ---------------
PSL_INIT_HD void psl_init_normalized(const PslInitRows* R, int r, const PslInitNorm* n1, const PslInitNorm* n2, float* p) {
    float q[4];
    psl_init_load(R, r, q);
    p[0] = (q[0] - n1->mx) * n1->sx; p[1] = (q[1] - n1->my) * n1->sy;
    p[2] = (q[2] - n2->mx) * n2->sx; p[3] = (q[3] - n2->my) * n2->sy;
}
template <int ES>
PSL_INIT_HD void psl_init_hyp_h(const PslInitRows* R, const int* idx, const PslInitNorm* n1, const PslInitNorm* n2, float* ws, double* wd,
                                float* H21, float* H12) {
    float* a = ws + (size_t)PSL_INIT_WS_A * ES;
    float* v = ws + (size_t)PSL_INIT_WS_V * ES;
    for (int i = 0; i < 8; ++i) {
        float p[4];
        psl_init_normalized(R, idx[i], n1, n2, p);
        const float u1 = p[0], v1 = p[1], u2 = p[2], v2 = p[3];
        const float r0[9] = {0.f, 0.f, 0.f, -u1, -v1, -1.f, v2 * u1, v2 * v1, v2};
        const float r1[9] = {u1, v1, 1.f, 0.f, 0.f, 0.f, -u2 * u1, -u2 * v1, -u2};
        for (int c = 0; c < 9; ++c) { F_(a, c * 16 + 2 * i) = r0[c]; F_(a, c * 16 + 2 * i + 1) = r1[c]; }
    }
    psl_init_jacobi<ES>(a, 16, 9, wd, v);
    float Hn[9], T1[9], T2[9], T2inv[9], t[9];
    for (int k = 0; k < 9; ++k) Hn[k] = F_(v, 8 * 9 + k);
    psl_init_T(n1, T1);
    psl_init_T(n2, T2);
    psl_init_inv3(T2, T2inv);
    psl_init_mul33(T2inv, Hn, t);
    psl_init_mul33(t, T1, H21);
    psl_init_inv3(H21, H12);
}
// ---- ComputeF21 (:268-303) + the de-normalisation (:212) -----------------------------------------------------------------------------
template <int ES>
PSL_INIT_HD void psl_init_hyp_f(const PslInitRows* R, const int* idx, const PslInitNorm* n1, const PslInitNorm* n2, float* ws, double* wd,
                                float* F21) {
    float* a = ws + (size_t)PSL_INIT_WS_A * ES;
    float* v = ws + (size_t)PSL_INIT_WS_V * ES;
    for (int i = 0; i < 8; ++i) {
        float p[4];
        psl_init_normalized(R, idx[i], n1, n2, p);
        const float u1 = p[0], v1 = p[1], u2 = p[2], v2 = p[3];
        const float r[9] = {u2 * u1, u2 * v1, u2, v2 * u1, v2 * v1, v2, u1, v1, 1.f};
        for (int c = 0; c < 9; ++c) F_(a, i * 9 + c) = r[c];
    }
    psl_init_jacobi<ES>(a, 9, 8, wd, (float*)nullptr);   // the 8x8 "V" side is never read
    psl_init_complete<ES>(a, 9, 8, 9, wd);
    float Fpre[9], u[9], wf[3], vt[9];
    for (int k = 0; k < 9; ++k) Fpre[k] = F_(a, 8 * 9 + k);
    psl_init_svd3<ES>(Fpre, a + (size_t)81 * ES, wd, v, u, wf, vt);
    wf[2] = 0.f;
    const float D[9] = {wf[0], 0.f, 0.f, 0.f, wf[1], 0.f, 0.f, 0.f, wf[2]};
    float t[9], Fn[9], T1[9], T2[9], T2t[9];
    psl_init_mul33(u, D, t);
    psl_init_mul33(t, vt, Fn);
    psl_init_T(n1, T1);
    psl_init_T(n2, T2);
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) T2t[3 * i + j] = T2[3 * j + i];
    psl_init_mul33(T2t, Fn, t);
    psl_init_mul33(t, T1, F21);
}

// ---- CheckHomography / CheckFundamental for one row (:337-385, :413-465): the row's terms are added to *score; returns bIn -------------
PSL_INIT_HD float psl_init_inv_sigma2(float sigma) { return (float)PSL_PO_DIV(1.0, (double)(sigma * sigma)); }
PSL_INIT_HD int psl_init_score_h(const float* H21, const float* H12, const float* q, float invSigmaSquare, float* score) {
    const float th = 5.991f;
    const float u1 = q[0], v1 = q[1], u2 = q[2], v2 = q[3];
    int bIn = 1;
    const float w2in1inv = (float)PSL_PO_DIV(1.0, (double)((H12[6] * u2 + H12[7] * v2) + H12[8]));
    const float u2in1 = ((H12[0] * u2 + H12[1] * v2) + H12[2]) * w2in1inv;
    const float v2in1 = ((H12[3] * u2 + H12[4] * v2) + H12[5]) * w2in1inv;
    const float squareDist1 = (u1 - u2in1) * (u1 - u2in1) + (v1 - v2in1) * (v1 - v2in1);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = 0;
    else *score = *score + (th - chiSquare1);
    const float w1in2inv = (float)PSL_PO_DIV(1.0, (double)((H21[6] * u1 + H21[7] * v1) + H21[8]));
    const float u1in2 = ((H21[0] * u1 + H21[1] * v1) + H21[2]) * w1in2inv;
    const float v1in2 = ((H21[3] * u1 + H21[4] * v1) + H21[5]) * w1in2inv;
    const float squareDist2 = (u2 - u1in2) * (u2 - u1in2) + (v2 - v1in2) * (v2 - v1in2);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = 0;
    else *score = *score + (th - chiSquare2);
    return bIn;
}
PSL_INIT_HD int psl_init_score_f(const float* F, const float* q, float invSigmaSquare, float* score) {
    const float th = 3.841f, thScore = 5.991f;
    const float u1 = q[0], v1 = q[1], u2 = q[2], v2 = q[3];
    int bIn = 1;
    const float a2 = (F[0] * u1 + F[1] * v1) + F[2];
    const float b2 = (F[3] * u1 + F[4] * v1) + F[5];
    const float c2 = (F[6] * u1 + F[7] * v1) + F[8];
    const float num2 = (a2 * u2 + b2 * v2) + c2;
    const float squareDist1 = PSL_RS_FDIV(num2 * num2, a2 * a2 + b2 * b2);
    const float chiSquare1 = squareDist1 * invSigmaSquare;
    if (chiSquare1 > th) bIn = 0;
    else *score = *score + (thScore - chiSquare1);
    const float a1 = (F[0] * u2 + F[3] * v2) + F[6];
    const float b1 = (F[1] * u2 + F[4] * v2) + F[7];
    const float c1 = (F[2] * u2 + F[5] * v2) + F[8];
    const float num1 = (a1 * u1 + b1 * v1) + c1;
    const float squareDist2 = PSL_RS_FDIV(num1 * num1, a1 * a1 + b1 * b1);
    const float chiSquare2 = squareDist2 * invSigmaSquare;
    if (chiSquare2 > th) bIn = 0;
    else *score = *score + (thScore - chiSquare2);
    return bIn;
}
// the flag of a row under the model of the branch that was taken; M: H21 (9) H12 (9), or F21 (9)
PSL_INIT_HD int psl_init_inlier(int homography, const float* M, const float* q, float invSigmaSquare) {
    float s = 0.f;
    return homography ? psl_init_score_h(M, M + 9, q, invSigmaSquare, &s) : psl_init_score_f(M, q, invSigmaSquare, &s);
}

// ---- the motion hypotheses ---------------------------------------------------------------------------------------------------------
PSL_INIT_HD void psl_init_K(const PslCamera* cam, float* K) {
    K[0] = cam->fx; K[1] = 0.f; K[2] = cam->cx;
    K[3] = 0.f; K[4] = cam->fy; K[5] = cam->cy;
    K[6] = 0.f; K[7] = 0.f; K[8] = 1.f;
}
// ReconstructF :479-487 with DecomposeE :909-929: hypothesis k = (R[k & 1], k < 2 ? t : -t) in Rs [4][9], ts [4][3]
template <int ES>
PSL_INIT_HD void psl_init_motion_f(const float* F21, const float* K, float* a, double* w, float* v, float* Rs, float* ts) {
    float E[9], tmp[9], u[9], wf[3], vt[9];
    psl_init_mul33_t(K, F21, 1, tmp);
    psl_init_mul33(tmp, K, E);
    psl_init_svd3<ES>(E, a, w, v, u, wf, vt);
    float t[3] = {u[2], u[5], u[8]};
    psl_init_unit3(t);
    const float W[9] = {0.f, -1.f, 0.f, 1.f, 0.f, 0.f, 0.f, 0.f, 1.f};
    float R1[9], R2[9];
    psl_init_mul33(u, W, tmp);
    psl_init_mul33(tmp, vt, R1);
    if (psl_init_det3(R1) < 0)
        for (int k = 0; k < 9; ++k) R1[k] = -R1[k];
    psl_init_mul33_t(u, W, 0, tmp);
    psl_init_mul33(tmp, vt, R2);
    if (psl_init_det3(R2) < 0)
        for (int k = 0; k < 9; ++k) R2[k] = -R2[k];
    for (int h = 0; h < 4; ++h) {
        for (int k = 0; k < 9; ++k) Rs[9 * h + k] = (h & 1) ? R2[k] : R1[k];
        for (int k = 0; k < 3; ++k) ts[3 * h + k] = h < 2 ? t[k] : -t[k];
    }
}
// ReconstructH :584-686: returns 0 at the d1/d2, d2/d3 gate (:597-600); Rs [8][9], ts [8][3]
template <int ES>
PSL_INIT_HD int psl_init_motion_h(const float* H21, const float* K, float* a, double* w, float* v, float* Rs, float* ts) {
    float invK[9], tmp[9], A[9], U[9], wf[3], Vt[9];
    psl_init_inv3(K, invK);
    psl_init_mul33(invK, H21, tmp);
    psl_init_mul33(tmp, K, A);
    psl_init_svd3<ES>(A, a, w, v, U, wf, Vt);
    const float s = (float)(psl_init_det3(U) * psl_init_det3(Vt));
    const float d1 = wf[0], d2 = wf[1], d3 = wf[2];
    if ((double)PSL_RS_FDIV(d1, d2) < 1.00001 || (double)PSL_RS_FDIV(d2, d3) < 1.00001) return 0;
    const float aux1 = PSL_INIT_FSQRT(PSL_RS_FDIV(d1 * d1 - d2 * d2, d1 * d1 - d3 * d3));
    const float aux3 = PSL_INIT_FSQRT(PSL_RS_FDIV(d2 * d2 - d3 * d3, d1 * d1 - d3 * d3));
    const float aux_stheta = PSL_RS_FDIV(PSL_INIT_FSQRT((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 + d3) * d2);
    const float ctheta = PSL_RS_FDIV(d2 * d2 + d1 * d3, (d1 + d3) * d2);
    const float aux_sphi = PSL_RS_FDIV(PSL_INIT_FSQRT((d1 * d1 - d2 * d2) * (d2 * d2 - d3 * d3)), (d1 - d3) * d2);
    const float cphi = PSL_RS_FDIV(d1 * d3 - d2 * d2, (d1 - d3) * d2);
    for (int h = 0; h < 8; ++h) {
        const int i = h & 3;   // x1 = {+, +, -, -} aux1, x3 = {+, -, +, -} aux3, stheta / sphi = {+, -, -, +} aux
        const float x1 = i < 2 ? aux1 : -aux1, x3 = (i & 1) ? -aux3 : aux3;
        const float st = (i == 0 || i == 3) ? aux_stheta : -aux_stheta, sp = (i == 0 || i == 3) ? aux_sphi : -aux_sphi;
        float Rp[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
        float tp[3];
        if (h < 4) {
            Rp[0] = ctheta; Rp[2] = -st; Rp[6] = st; Rp[8] = ctheta;
            tp[0] = x1 * (d1 - d3); tp[1] = 0.f * (d1 - d3); tp[2] = -x3 * (d1 - d3);
        } else {
            Rp[0] = cphi; Rp[2] = sp; Rp[4] = -1.f; Rp[6] = sp; Rp[8] = -cphi;
            tp[0] = x1 * (d1 + d3); tp[1] = 0.f * (d1 + d3); tp[2] = x3 * (d1 + d3);
        }
        psl_init_mul33(U, Rp, tmp);
        for (int k = 0; k < 9; ++k) tmp[k] = tmp[k] * s;
        psl_init_mul33(tmp, Vt, Rs + 9 * h);
        float t[3];
        psl_init_mul31(U, tp, t);
        psl_init_unit3(t);
        for (int k = 0; k < 3; ++k) ts[3 * h + k] = t[k];
    }
    return 1;
}

// ---- CheckRT (:798-907): the set-up of one hypothesis, one row, the parallax ----------------------------------------------------------
struct PslInitRt {
    float R[9], t[3], P1[12], P2[12], O2[3];
    float fx, fy, cx, cy, th2;
};
PSL_INIT_HD void psl_init_rt_setup(const float* R, const float* t, const float* K, float th2, PslInitRt* S) {
    for (int k = 0; k < 9; ++k) S->R[k] = R[k];
    for (int k = 0; k < 3; ++k) S->t[k] = t[k];
    S->fx = K[0]; S->fy = K[4]; S->cx = K[2]; S->cy = K[5]; S->th2 = th2;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 4; ++j) {
            S->P1[4 * i + j] = j < 3 ? K[3 * i + j] : 0.f;
            const float r0 = j < 3 ? R[j] : t[0], r1 = j < 3 ? R[3 + j] : t[1], r2 = j < 3 ? R[6 + j] : t[2];
            S->P2[4 * i + j] = (K[3 * i] * r0 + K[3 * i + 1] * r1) + K[3 * i + 2] * r2;
        }
    for (int i = 0; i < 3; ++i) {   // O2 = -R.t()*t
        double s = 0.0;
        for (int k = 0; k < 3; ++k) s = s + (double)R[3 * k + i] * (double)t[k];
        S->O2[i] = (float)(s * -1.0);
    }
}
// One row whose flag is set: 0 = not counted; 1 = counted in nGood (p -> vP3D, *cosp -> vCosParallax); 3 = also vbGood.
// a: PSL_INIT_RT_F floats, w: PSL_INIT_RT_D doubles of workspace
template <int ES>
PSL_INIT_HD int psl_init_rt_row(const PslInitRt* S, const float* q, float* a, double* w, float* p, float* cosp) {
    float* v = a + (size_t)16 * ES;
    // Triangulate (:734-747); At = A^T
    for (int j = 0; j < 4; ++j) {
        F_(a, 4 * j + 0) = q[0] * S->P1[8 + j] - S->P1[j];
        F_(a, 4 * j + 1) = q[1] * S->P1[8 + j] - S->P1[4 + j];
        F_(a, 4 * j + 2) = q[2] * S->P2[8 + j] - S->P2[j];
        F_(a, 4 * j + 3) = q[3] * S->P2[8 + j] - S->P2[4 + j];
    }
    psl_init_jacobi<ES>(a, 4, 4, w, v);
    const double inv = PSL_PO_DIV(1.0, (double)F_(v, 15));
    for (int k = 0; k < 3; ++k) p[k] = (float)((double)F_(v, 12 + k) * inv);
    const float inf = __builtin_inff();
    if (!(__builtin_fabsf(p[0]) < inf) || !(__builtin_fabsf(p[1]) < inf) || !(__builtin_fabsf(p[2]) < inf)) return 0;
    const float dist1 = (float)PSL_PO_SQRT(((double)p[0] * (double)p[0] + (double)p[1] * (double)p[1]) + (double)p[2] * (double)p[2]);
    const float n2[3] = {p[0] - S->O2[0], p[1] - S->O2[1], p[2] - S->O2[2]};
    const float dist2 = (float)PSL_PO_SQRT(((double)n2[0] * (double)n2[0] + (double)n2[1] * (double)n2[1]) + (double)n2[2] * (double)n2[2]);
    const double dot = ((double)p[0] * (double)n2[0] + (double)p[1] * (double)n2[1]) + (double)p[2] * (double)n2[2];
    const float cosParallax = (float)PSL_PO_DIV(dot, (double)(dist1 * dist2));
    *cosp = cosParallax;
    if (p[2] <= 0 && (double)cosParallax < 0.99998) return 0;
    float p2[3];
    psl_init_mul31(S->R, p, p2);
    for (int k = 0; k < 3; ++k) p2[k] = p2[k] + S->t[k];
    if (p2[2] <= 0 && (double)cosParallax < 0.99998) return 0;
    const float invZ1 = (float)PSL_PO_DIV(1.0, (double)p[2]);
    const float im1x = (S->fx * p[0]) * invZ1 + S->cx, im1y = (S->fy * p[1]) * invZ1 + S->cy;
    const float squareError1 = (im1x - q[0]) * (im1x - q[0]) + (im1y - q[1]) * (im1y - q[1]);
    if (squareError1 > S->th2) return 0;
    const float invZ2 = (float)PSL_PO_DIV(1.0, (double)p2[2]);
    const float im2x = (S->fx * p2[0]) * invZ2 + S->cx, im2y = (S->fy * p2[1]) * invZ2 + S->cy;
    const float squareError2 = (im2x - q[2]) * (im2x - q[2]) + (im2y - q[3]) * (im2y - q[3]);
    if (squareError2 > S->th2) return 0;
    return (double)cosParallax < 0.99998 ? 3 : 1;
}
// the order of vCosParallax: ascending keys
PSL_INIT_HD uint32_t psl_init_cos_key(float c) {
    uint32_t b;
    __builtin_memcpy(&b, &c, 4);
    return (b >> 31) ? ~b : (b | 0x80000000u);
}
PSL_INIT_HD float psl_init_cos_unkey(uint32_t k) {
    const uint32_t b = (k >> 31) ? (k & 0x7fffffffu) : ~k;
    float c;
    __builtin_memcpy(&c, &b, 4);
    return c;
}
// :896-904 from the element at sorted index min(50, size - 1): acosf, a float product, a double division
PSL_INIT_HD float psl_init_parallax(float cosv) { return (float)PSL_PO_DIV((double)(psl_acosf(cosv) * 180.f), PSL_INIT_PI); }

// ---- the decision trees --------------------------------------------------------------------------------------------------------------
// ReconstructF :499-569: returns 1 when Initialize is true; *best = the hypothesis of the else-if ladder, -1 when it is not reached
PSL_INIT_HD int psl_init_decide_f(const int* g, const float* par, int N, float minParallax, int minTriangulated, int* best) {
    int maxGood = g[3];
    if (g[2] > maxGood) maxGood = g[2];
    if (g[1] > maxGood) maxGood = g[1];
    if (g[0] > maxGood) maxGood = g[0];
    int nMinGood = (int)(0.9 * (double)N);
    if (nMinGood < minTriangulated) nMinGood = minTriangulated;
    int nsimilar = 0;
    for (int k = 0; k < 4; ++k)
        if ((double)g[k] > 0.7 * (double)maxGood) ++nsimilar;
    *best = -1;
    if (maxGood < nMinGood || nsimilar > 1) return 0;
    const int k = maxGood == g[0] ? 0 : (maxGood == g[1] ? 1 : (maxGood == g[2] ? 2 : 3));
    *best = k;
    return par[k] > minParallax ? 1 : 0;
}
// ReconstructH :689-731: *best = bestSolutionIdx
PSL_INIT_HD int psl_init_decide_h(const int* g, const float* par, int N, float minParallax, int minTriangulated, int* best) {
    int bestGood = 0, secondBestGood = 0, bestIdx = -1;
    float bestParallax = -1.f;
    for (int i = 0; i < 8; ++i) {
        if (g[i] > bestGood) {
            secondBestGood = bestGood; bestGood = g[i]; bestIdx = i; bestParallax = par[i];
        } else if (g[i] > secondBestGood) {
            secondBestGood = g[i];
        }
    }
    *best = bestIdx;
    return ((double)secondBestGood < 0.75 * (double)bestGood && bestParallax >= minParallax && bestGood > minTriangulated &&
            (double)bestGood > 0.9 * (double)N) ? 1 : 0;
}
PSL_INIT_HD float psl_init_th2(float sigma) { return (float)(4.0 * (double)(sigma * sigma)); }

#ifndef __HIP_DEVICE_COMPILE__
// ---- Initialize (:44-121) on one core -------------------------------------------------------------------------------------------------
// keys: x, y at a stride of ks floats; matches12 [n1]; p3d [n1][3], tri [n1] and (may be NULL) matches_out [n1] are written in full.
// ws: PSL_INIT_WS_F floats, wd: PSL_INIT_WS_D doubles, row_i: n1 ints of workspace, keybuf: n1 uint32 of workspace.
// the key at sorted index min(50, n - 1) (:898-900), n >= 1: a selection sort of the first places; keybuf is reordered
static inline uint32_t psl_init_select_key(uint32_t* keybuf, int n) {
    const int idx = n - 1 < 50 ? n - 1 : 50;
    for (int i = 0; i <= idx; ++i) {
        int m = i;
        for (int j = i + 1; j < n; ++j)
            if (keybuf[j] < keybuf[m]) m = j;
        const uint32_t tk = keybuf[i]; keybuf[i] = keybuf[m]; keybuf[m] = tk;
    }
    return keybuf[idx];
}
static inline int psl_init_check_rt_host(const PslInitRows* R, int N, int homography, const float* M, float invS2, const float* Rm, const float* t,
                                         const float* K, float th2, float* ws, double* wd, uint32_t* keybuf, float* p3d, uint8_t* tri,
                                         float* parallax) {
    PslInitRt S;
    psl_init_rt_setup(Rm, t, K, th2, &S);
    int nGood = 0;
    for (int r = 0; r < N; ++r) {
        float q[4], p[3], cosp = 0.f;
        const int i1 = psl_init_load(R, r, q);
        if (!psl_init_inlier(homography, M, q, invS2)) continue;
        const int c = psl_init_rt_row<1>(&S, q, ws, wd, p, &cosp);
        if (!c) continue;
        keybuf[nGood++] = psl_init_cos_key(cosp);
        if (p3d) {
            p3d[3 * (size_t)i1] = p[0]; p3d[3 * (size_t)i1 + 1] = p[1]; p3d[3 * (size_t)i1 + 2] = p[2];
            if (c == 3) tri[i1] = 1;
        }
    }
    *parallax = nGood > 0 ? psl_init_parallax(psl_init_cos_unkey(psl_init_select_key(keybuf, nGood))) : 0.f;
    return nGood;
}

static inline void psl_init_initialize_host(const float* k1, int n1, const float* k2, int n2, size_t ks, const int32_t* matches12,
                                            const PslCamera* cam, float sigma, int max_its, uint32_t seed, float* ws, double* wd,
                                            int32_t* row_i, uint32_t* keybuf, PslInitResult* res, float* p3d, uint8_t* tri,
                                            int32_t* matches_out) {
    memset(res, 0, sizeof(*res));
    res->best_it_h = res->best_it_f = res->best_hypothesis = -1;
    for (int i = 0; i < n1; ++i) {
        p3d[3 * (size_t)i] = p3d[3 * (size_t)i + 1] = p3d[3 * (size_t)i + 2] = 0.f;
        tri[i] = 0;
        if (matches_out) matches_out[i] = matches12[i];
    }
    int N = 0;
    for (int i = 0; i < n1; ++i) {
        if (matches12[i] >= n2) {   // a match outside frame 2: the record alone says so
            memset(res, 0, sizeof(*res));
            res->status = PSLFE_E_INVALID;
            return;
        }
        if (matches12[i] >= 0) row_i[N++] = i;
    }
    res->nmatches = N;
    if (N < 8) return;
    const PslInitRows R = {nullptr, 0, row_i, matches12, k1, k2, ks};
    PslInitNorm nm1, nm2;
    psl_init_normalize(k1, ks, n1, 0, &nm1.mx, &nm1.sx);
    psl_init_normalize(k1, ks, n1, 1, &nm1.my, &nm1.sy);
    psl_init_normalize(k2, ks, n2, 0, &nm2.mx, &nm2.sx);
    psl_init_normalize(k2, ks, n2, 1, &nm2.my, &nm2.sy);
    const float invS2 = psl_init_inv_sigma2(sigma);
    PslRsRand G;
    psl_rs_srand(&G, seed);
    float SH = 0.f, SF = 0.f, MH[18], MF[9];
    for (int it = 0; it < max_its; ++it) {
        int idx[8];
        psl_rs_draw<8>(&G, N, idx);
        float H21[9], H12[9], F21[9], sh = 0.f, sf = 0.f;
        psl_init_hyp_h<1>(&R, idx, &nm1, &nm2, ws, wd, H21, H12);
        psl_init_hyp_f<1>(&R, idx, &nm1, &nm2, ws, wd, F21);
        for (int r = 0; r < N; ++r) {
            float q[4];
            psl_init_load(&R, r, q);
            psl_init_score_h(H21, H12, q, invS2, &sh);
            psl_init_score_f(F21, q, invS2, &sf);
        }
        if (sh > SH) { SH = sh; res->best_it_h = it; for (int k = 0; k < 9; ++k) { MH[k] = H21[k]; MH[9 + k] = H12[k]; } }
        if (sf > SF) { SF = sf; res->best_it_f = it; for (int k = 0; k < 9; ++k) MF[k] = F21[k]; }
    }
    res->SH = SH; res->SF = SF;
    for (int r = 0; r < N; ++r) {
        float q[4];
        psl_init_load(&R, r, q);
        if (res->best_it_h >= 0) res->inliers_h += psl_init_inlier(1, MH, q, invS2);
        if (res->best_it_f >= 0) res->inliers_f += psl_init_inlier(0, MF, q, invS2);
    }
    if (res->best_it_h >= 0) for (int k = 0; k < 9; ++k) res->H21[k] = MH[k];
    if (res->best_it_f >= 0) for (int k = 0; k < 9; ++k) res->F21[k] = MF[k];
    if (res->best_it_h < 0 && res->best_it_f < 0) { res->status = 4; return; }
    res->RH = PSL_RS_FDIV(SH, SH + SF);
    const int homography = (double)res->RH > 0.40;
    if (homography) res->status |= 2;
    float K[9], Rs[72], ts[24];
    psl_init_K(cam, K);
    const float th2 = psl_init_th2(sigma);
    const float* M = homography ? MH : MF;
    const int nin = homography ? res->inliers_h : res->inliers_f;
    int nh = 4;
    if (homography) {
        if (!psl_init_motion_h<1>(MH, K, ws, wd, ws + 9, Rs, ts)) return;
        nh = 8;
    } else {
        psl_init_motion_f<1>(MF, K, ws, wd, ws + 9, Rs, ts);
    }
    for (int h = 0; h < nh; ++h)
        res->ngood[h] = psl_init_check_rt_host(&R, N, homography, M, invS2, Rs + 9 * h, ts + 3 * h, K, th2, ws, wd, keybuf, nullptr, nullptr,
                                               &res->parallax[h]);
    int best = -1;
    const int ok = homography ? psl_init_decide_h(res->ngood, res->parallax, nin, 1.0f, 50, &best)
                              : psl_init_decide_f(res->ngood, res->parallax, nin, 1.0f, 50, &best);
    res->best_hypothesis = best;
    if (!ok) return;
    res->status |= 1;
    float par;
    psl_init_check_rt_host(&R, N, homography, M, invS2, Rs + 9 * best, ts + 3 * best, K, th2, ws, wd, keybuf, p3d, tri, &par);
    for (int k = 0; k < 9; ++k) res->R21[k] = Rs[9 * best + k];
    for (int k = 0; k < 3; ++k) res->t21[k] = ts[3 * best + k];
    for (int i = 0; i < n1; ++i) {
        res->ntriangulated += tri[i];
        if (matches_out && matches12[i] >= 0 && !tri[i]) matches_out[i] = -1;
    }
}
#endif

#undef F_
#endif
