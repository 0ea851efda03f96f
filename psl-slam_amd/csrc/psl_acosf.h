// Plain C++ text, next to psl_atanf.h.  Product code.
#ifndef PSL_ACOSF_H
#define PSL_ACOSF_H
// libm acosf as Initializer::CheckRT calls it (src/Initializer.cc:901: acos on a float with `using namespace std` in scope): the
// fdlibm algorithm (e_acosf.c), plain f32 arithmetic, restated.  Newer glibc versions ship a correctly rounded acosf instead;
// tests/test_initializer_cpu.py measures the deviation from the host's acosf on a grid.  Only the comparison of
// the parallax with minParallax consumes the value.  The caller defines PSL_ACOSF_HD, PSL_ACOSF_DIV (a correctly rounded float
// division) and PSL_ACOSF_SQRT (a correctly rounded float square root); every other operation is a single float operation under
// -ffp-contract=off.
#ifdef __clang__
#pragma clang fp contract(off)
#endif
PSL_ACOSF_HD float psl_acosf(float x) {
    const float one = 1.0000000000e+00f, pi = 3.1415925026e+00f, pio2_hi = 1.5707962513e+00f, pio2_lo = 7.5497894159e-08f,
                pS0 = 1.6666667163e-01f, pS1 = -3.2556581497e-01f, pS2 = 2.0121252537e-01f, pS3 = -4.0055535734e-02f,
                pS4 = 7.9153501429e-04f, pS5 = 3.4793309169e-05f, qS1 = -2.4033949375e+00f, qS2 = 2.0209457874e+00f,
                qS3 = -6.8828397989e-01f, qS4 = 7.7038154006e-02f;
    int32_t hx;
    __builtin_memcpy(&hx, &x, 4);
    const int32_t ix = hx & 0x7fffffff;
    if (ix == 0x3f800000) return hx > 0 ? 0.0f : pi + 2.0f * pio2_lo;   // |x| == 1
    if (ix > 0x3f800000) return PSL_ACOSF_DIV(x - x, x - x);            // |x| > 1 or NaN: NaN
    if (ix < 0x3f000000) {                                              // |x| < 0.5
        if (ix <= 0x23000000) return pio2_hi + pio2_lo;
        const float z = x * x;
        const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const float q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const float r = PSL_ACOSF_DIV(p, q);
        return pio2_hi - (x - (pio2_lo - x * r));
    }
    if (hx < 0) {                                                       // x < -0.5
        const float z = (one + x) * 0.5f;
        const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
        const float q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
        const float s = PSL_ACOSF_SQRT(z);
        const float r = PSL_ACOSF_DIV(p, q);
        const float w = r * s - pio2_lo;
        return pi - 2.0f * (s + w);
    }
    const float z = (one - x) * 0.5f;                                   // x > 0.5
    const float s = PSL_ACOSF_SQRT(z);
    float df = s;
    int32_t idf;
    __builtin_memcpy(&idf, &df, 4);
    idf &= (int32_t)0xfffff000;
    __builtin_memcpy(&df, &idf, 4);
    const float c = PSL_ACOSF_DIV(z - df * df, s + df);
    const float p = z * (pS0 + z * (pS1 + z * (pS2 + z * (pS3 + z * (pS4 + z * pS5)))));
    const float q = one + z * (qS1 + z * (qS2 + z * (qS3 + z * qS4)));
    const float r = PSL_ACOSF_DIV(p, q);
    const float w = r * s + c;
    return 2.0f * (df + w);
}
#endif
