// ORACLE (test infrastructure only - never linked into the product library).
// Host twins of pslfe_debug_math (psl-slam_amd/csrc/pslfe_debug_math.hip): the HOST compile of the product's own restated libm -
// psl_device_math.h (+ psl_atanf.h), psl_sincos64.h, psl_sincos_glibc.h, psl_f64math.h, psl_log_gamma.h - evaluated on caller-supplied
// arguments, with the function ids of include/pslfe.h.  The GPU tests demand that the device returns the same bytes
// (tests/test_debug_math_gpu.py).  Built like the rest of the oracle: -O2 -ffp-contract=off, every operation a single IEEE operation;
// __builtin_fma compiles to the hardware instruction or to libm's fma(), both correctly rounded (no -mfma: the library travels).
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "../include/pslfe.h"                           // the PSLFE_MATH_* ids
#include "../psl-slam_amd/csrc/psl_device_math.h"       // without hipcc: its host half alone
#define PSL_SC64_QUAL static inline
#include "../psl-slam_amd/csrc/psl_sincos64.h"
#include "../psl-slam_amd/csrc/psl_sincos_glibc.h"
#define PSL_F64_QUAL static inline
#include "../psl-slam_amd/csrc/psl_f64math.h"
#include "../psl-slam_amd/csrc/psl_log_gamma.h"

#if defined(__HIP_DEVICE_COMPILE__) || defined(__FAST_MATH__)
#error "math_oracle.cpp is the plain host compile of the product's math headers"
#endif

namespace {
const double SCTAB[444] = {
#include "../psl-slam_amd/csrc/psl_sincostab.inc"
};
}  // namespace

extern "C" {

// out0 / out1 as pslfe_debug_math writes them; returns 0, or -1 for an unknown id or a missing array
int pso_math_eval(int fn, size_t n, const void* a, const void* b, void* out0, void* out1) {
    const float* af = (const float*)a;
    const float* bf = (const float*)b;
    const double* ad = (const double*)a;
    const double* bd = (const double*)b;
    float* of0 = (float*)out0;
    float* of1 = (float*)out1;
    double* od0 = (double*)out0;
    double* od1 = (double*)out1;
    int32_t* oi0 = (int32_t*)out0;
    if (fn < 0 || fn >= PSLFE_MATH_COUNT) return -1;
    if (n == 0) return 0;
    const bool binary = fn == PSLFE_MATH_FAST_ATAN2 || fn == PSLFE_MATH_ATAN2F || fn == PSLFE_MATH_FDIV || fn == PSLFE_MATH_POW_POS ||
                        fn == PSLFE_MATH_RATIO_INV || fn == PSLFE_MATH_DDIV;
    const bool two = fn == PSLFE_MATH_SINCOSF || fn == PSLFE_MATH_COS_SIN_F64 || fn == PSLFE_MATH_COS_SIN_2PI_F32;
    if (!a || !out0 || (binary && !b) || (two && !out1)) return -1;
    for (size_t i = 0; i < n; ++i) {
        switch (fn) {
            case PSLFE_MATH_ATANF: of0[i] = psl_atanf(af[i]); break;
            case PSLFE_MATH_TANF: of0[i] = psl_tanf(af[i]); break;
            case PSLFE_MATH_SINCOSF: { float s, c; psl_sincosf(af[i], &s, &c); of0[i] = s; of1[i] = c; break; }
            case PSLFE_MATH_FAST_ATAN2: of0[i] = psl_fast_atan2(af[i], bf[i]); break;
            case PSLFE_MATH_ATAN2F: of0[i] = psl_atan2f(af[i], bf[i]); break;
            case PSLFE_MATH_FDIV: of0[i] = PSL_FDIV(af[i], bf[i]); break;
            case PSLFE_MATH_SQRTF: of0[i] = __builtin_sqrtf(af[i]); break;
            case PSLFE_MATH_CVROUND_F: oi0[i] = psl_cvround_f(af[i]); break;
            case PSLFE_MATH_LOG: od0[i] = psl_log(ad[i]); break;
            case PSLFE_MATH_EXP: od0[i] = psl_exp(ad[i]); break;
            case PSLFE_MATH_LOG10: od0[i] = psl_log10(ad[i]); break;
            case PSLFE_MATH_POW_POS: od0[i] = psl_pow_pos(ad[i], bd[i]); break;
            case PSLFE_MATH_SINH_SMALL: od0[i] = psl_sinh_small(ad[i]); break;
            case PSLFE_MATH_LOG_GAMMA: od0[i] = lsdn_log_gamma(ad[i]); break;
            case PSLFE_MATH_GLIBC_SIN: od0[i] = psl_glibc_sin(ad[i], SCTAB); break;
            case PSLFE_MATH_GLIBC_COS: od0[i] = psl_glibc_cos(ad[i], SCTAB); break;
            case PSLFE_MATH_COS_SIN_F64: { double c, s; psl_cos_sin_f64(ad[i], &c, &s); od0[i] = c; od1[i] = s; break; }
            case PSLFE_MATH_COS_SIN_2PI_F32: { float c, s; psl_cos_sin_2pi_f32(ad[i], &c, &s); of0[i] = c; of1[i] = s; break; }
            case PSLFE_MATH_RATIO_INV: od0[i] = psl_ratio_inv(ad[i], bd[i], 1.0 / bd[i]); break;
            case PSLFE_MATH_DDIV: od0[i] = ad[i] / bd[i]; break;
            case PSLFE_MATH_DSQRT: od0[i] = sqrt(ad[i]); break;
            case PSLFE_MATH_CVROUND_D: oi0[i] = psl_cvround_d(ad[i]); break;
        }
    }
    return 0;
}

}  // extern "C"
