// libpslfe: pslfe_debug_math - the restated libm of the kernels (psl_f64math.h, psl_sincos_glibc.h, psl_sincos64.h, psl_atanf.h,
// psl_device_math.h, psl_log_gamma.h) evaluated ON THE DEVICE on caller-supplied arguments.  Product code, built with the flags of
// every other kernel file (build.py): what this kernel returns for an argument is what a product kernel computes for it.  The
// tests compare it bit for bit with the host compile of the same headers (oracle/math_oracle.cpp).
#include "pslfe_internal.h"
#include "psl_device_math.h"
#define PSL_SC64_QUAL __host__ __device__ static inline
#include "psl_sincos64.h"
#include "psl_sincos_glibc.h"
#define PSL_F64_QUAL __host__ __device__ static inline
#include "psl_f64math.h"
#include "psl_log_gamma.h"

// the table of psl_glibc_sin / psl_glibc_cos in HBM, as the line kernels read theirs (LineParams.sctab)
__device__ const double g_dbg_sctab[444] = {
#include "psl_sincostab.inc"
};

__global__ __launch_bounds__(256) void k_debug_math(int fn, size_t n, const void* __restrict__ a, const void* __restrict__ b, void* __restrict__ out0,
                                                    void* __restrict__ out1) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float* af = (const float*)a;
    const float* bf = (const float*)b;
    const double* ad = (const double*)a;
    const double* bd = (const double*)b;
    float* of0 = (float*)out0;
    float* of1 = (float*)out1;
    double* od0 = (double*)out0;
    double* od1 = (double*)out1;
    int32_t* oi0 = (int32_t*)out0;
    switch (fn) {   // uniform
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
        case PSLFE_MATH_GLIBC_SIN: od0[i] = psl_glibc_sin(ad[i], g_dbg_sctab); break;
        case PSLFE_MATH_GLIBC_COS: od0[i] = psl_glibc_cos(ad[i], g_dbg_sctab); break;
        case PSLFE_MATH_COS_SIN_F64: { double c, s; psl_cos_sin_f64(ad[i], &c, &s); od0[i] = c; od1[i] = s; break; }
        case PSLFE_MATH_COS_SIN_2PI_F32: { float c, s; psl_cos_sin_2pi_f32(ad[i], &c, &s); of0[i] = c; of1[i] = s; break; }
        case PSLFE_MATH_RATIO_INV: od0[i] = psl_ratio_inv(ad[i], bd[i], 1.0 / bd[i]); break;
        case PSLFE_MATH_DDIV: od0[i] = ad[i] / bd[i]; break;
        case PSLFE_MATH_DSQRT: od0[i] = sqrt(ad[i]); break;
        case PSLFE_MATH_CVROUND_D: oi0[i] = psl_cvround_d(ad[i]); break;
        default: break;
    }
}

namespace {
// element sizes of a function id: inputs, out0, out1 (0 = not used); binary = reads b
struct MathSig { int in, o0, o1, binary; };
bool math_sig(int fn, MathSig* s) {
    switch (fn) {
        case PSLFE_MATH_ATANF: case PSLFE_MATH_TANF: case PSLFE_MATH_SQRTF: case PSLFE_MATH_CVROUND_F: *s = {4, 4, 0, 0}; return true;
        case PSLFE_MATH_SINCOSF: *s = {4, 4, 4, 0}; return true;
        case PSLFE_MATH_FAST_ATAN2: case PSLFE_MATH_ATAN2F: case PSLFE_MATH_FDIV: *s = {4, 4, 0, 1}; return true;
        case PSLFE_MATH_LOG: case PSLFE_MATH_EXP: case PSLFE_MATH_LOG10: case PSLFE_MATH_SINH_SMALL: case PSLFE_MATH_LOG_GAMMA:
        case PSLFE_MATH_GLIBC_SIN: case PSLFE_MATH_GLIBC_COS: case PSLFE_MATH_DSQRT: *s = {8, 8, 0, 0}; return true;
        case PSLFE_MATH_POW_POS: case PSLFE_MATH_RATIO_INV: case PSLFE_MATH_DDIV: *s = {8, 8, 0, 1}; return true;
        case PSLFE_MATH_COS_SIN_F64: *s = {8, 8, 8, 0}; return true;
        case PSLFE_MATH_COS_SIN_2PI_F32: *s = {8, 4, 4, 0}; return true;
        case PSLFE_MATH_CVROUND_D: *s = {8, 4, 0, 0}; return true;
        default: return false;
    }
}
}  // namespace

extern "C" int pslfe_debug_math(pslfe_ctx* ctx, int fn, size_t n, const void* a, const void* b, void* out0, void* out1) {
    PSL_REQUIRE(ctx, PSLFE_E_INVALID, "pslfe_debug_math: ctx is NULL");
    MathSig s;
    PSL_REQUIRE(math_sig(fn, &s), PSLFE_E_INVALID, "pslfe_debug_math: unknown function id %d", fn);
    if (n == 0) return PSLFE_OK;
    PSL_REQUIRE(a && out0 && (!s.binary || b) && (!s.o1 || out1), PSLFE_E_INVALID, "pslfe_debug_math: NULL argument (function id %d)", fn);
    PSL_REQUIRE(n <= ((size_t)1 << 30), PSLFE_E_INVALID, "pslfe_debug_math: %zu elements (at most 2^30 per call)", n);
    PSL_HIP(hipSetDevice(ctx->device));
    hipStream_t st = ctx->stream;
    PslDeviceBuffers mem;   // freed on every return
    char *d_a = nullptr, *d_b = nullptr, *d_o0 = nullptr, *d_o1 = nullptr;
    mem.alloc(d_a, n * s.in, "a");
    if (s.binary) mem.alloc(d_b, n * s.in, "b");
    mem.alloc(d_o0, n * s.o0, "out0");
    if (s.o1) mem.alloc(d_o1, n * s.o1, "out1");
    if (int rc = mem.check("pslfe_debug_math")) return rc;
    PSL_HIP(hipMemcpyAsync(d_a, a, n * s.in, hipMemcpyHostToDevice, st));
    if (s.binary) PSL_HIP(hipMemcpyAsync(d_b, b, n * s.in, hipMemcpyHostToDevice, st));
    k_debug_math<<<(unsigned)((n + 255) / 256), 256, 0, st>>>(fn, n, d_a, d_b, d_o0, d_o1);
    PSL_HIP(hipGetLastError());
    PSL_HIP(hipMemcpyAsync(out0, d_o0, n * s.o0, hipMemcpyDeviceToHost, st));
    if (s.o1) PSL_HIP(hipMemcpyAsync(out1, d_o1, n * s.o1, hipMemcpyDeviceToHost, st));
    PSL_HIP(hipStreamSynchronize(st));
    return PSLFE_OK;
}
