// log_gamma() of LSD's nfa() (OpenCV 3.x lsd.cpp; twin in the reference tree: Thirdparty/line_descriptor/src/ED_Lib/NFA.cpp:106-160)
// over the restated libm of psl_f64math.h.  Product code: the host builds the log_gamma table of nfa() with it (pslfe_line.hip:
// allocate), the kernels evaluate it for arguments beyond that table (line_kernels3.h: lsdn_lg) and pslfe_debug_math.hip runs it on
// caller-supplied arguments.  Include psl_device_math.h (PSL_DMUL ..., PSL_HD) and psl_f64math.h first.
#ifndef PSL_LOG_GAMMA_H
#define PSL_LOG_GAMMA_H

// pow(x, n) for the integer-valued arguments log_gamma sees: exact products where libm's pow is exact as well (x <= 15,
// n <= 6); x^6 = (x^3)^2 with x^3 exact, i.e. one rounding - what a pow with < 1 ulp of error returns - for the Windschitl term
__host__ __device__ static inline double lsdn_log_gamma(double x) {
    if (x > 15.0) {
        const double c = PSL_DMUL(PSL_DMUL(x, x), x), x6 = PSL_DMUL(c, c);
        const double inner = PSL_DADD(PSL_DMUL(x, psl_sinh_small(1 / x)), 1 / PSL_DMUL(810.0, x6));
        return PSL_DADD(PSL_DSUB(PSL_DADD(0.918938533204673, PSL_DMUL(PSL_DSUB(x, 0.5), psl_log(x))), x), PSL_DMUL(PSL_DMUL(0.5, x), psl_log(inner)));
    }
    const double q[7] = {75122.6331530, 80916.6278952, 36308.2951477, 8687.24529705, 1168.92649479, 83.8676043424, 2.50662827511};
    double a = PSL_DSUB(PSL_DMUL(PSL_DADD(x, 0.5), psl_log(PSL_DADD(x, 5.5))), PSL_DADD(x, 5.5));
    double b = 0, xn = 1;
#pragma unroll
    for (int n = 0; n < 7; ++n) {
        a = PSL_DSUB(a, psl_log(PSL_DADD(x, (double)n)));
        b = PSL_DADD(b, PSL_DMUL(q[n], xn));
        xn = PSL_DMUL(xn, x);
    }
    return PSL_DADD(a, psl_log(b));
}

#endif
