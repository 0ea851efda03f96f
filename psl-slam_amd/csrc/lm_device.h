// Device only: steps 2 and 3 of the order of the sums (the headers of pslfe_pose.hip and pslfe_sim3.hip) on a workgroup of
// PSL_LM_LANES threads, shared by k_pose_optimize and k_sim3_optimize, and PslLmWorkgroup, the executor of psl_lm_levenberg on such
// a workgroup, shared by k_ba_local and k_eg_optimize.  On one core: psl_lm_reduce_lanes and PslLmSerial of lm_kernels.h.
#ifndef PSL_LM_DEVICE_H
#define PSL_LM_DEVICE_H

#include "lm_kernels.h"

// N values per thread: the butterfly inside each wave, then ((G0 + G1) + G2) + G3 of the four wave sums through LDS.  s_red holds
// two buffers of 4 * STRIDE doubles (STRIDE >= N: the kernel's number of sums); `flip` alternates them, so one barrier per reduction
// is enough.  Every thread calls it and gets the sums.
template <int N, int STRIDE>
__device__ __forceinline__ void psl_lm_reduce(double* acc, double* s_red, int& flip) {
#pragma unroll
    for (int k = 0; k < N; ++k) {
        double v = acc[k];
#pragma unroll
        for (int s = PSL_LM_GROUP / 2; s >= 1; s >>= 1) v = __dadd_rn(v, __shfl_down(v, s, PSL_LM_GROUP));
        acc[k] = v;
    }
    double* buf = s_red + flip * (4 * STRIDE);
    const int lane = threadIdx.x & (PSL_LM_GROUP - 1), w = threadIdx.x / PSL_LM_GROUP;
    if (lane == 0) {
#pragma unroll
        for (int k = 0; k < N; ++k) buf[w * STRIDE + k] = acc[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < N; ++k) acc[k] = __dadd_rn(__dadd_rn(__dadd_rn(buf[k], buf[STRIDE + k]), buf[2 * STRIDE + k]), buf[3 * STRIDE + k]);
    flip ^= 1;
}

// The executor of lm_kernels.h (its contract is above psl_lm_levenberg) on a workgroup of PSL_LM_LANES threads: a step ends with a
// barrier.  s_red: 2 * 4 doubles of LDS.
struct PslLmWorkgroup {
    double* s_red;
    int flip;
    template <class Fn>
    __device__ __forceinline__ void par(int n, Fn f) {
        for (int i = threadIdx.x; i < n; i += PSL_LM_LANES) f(i);
        __syncthreads();
    }
    template <class Fn>
    __device__ __forceinline__ void one(Fn f) {
        if (threadIdx.x == 0) f();
        __syncthreads();
    }
    template <class Fn>
    __device__ __forceinline__ double sum256(Fn f) {
        double v[1] = {f((int)threadIdx.x)};
        psl_lm_reduce<1, 1>(v, s_red, flip);
        return v[0];
    }
    template <class V>
    __device__ __forceinline__ V get(const V* p) {
        const V v = *(const volatile V*)p;
        __syncthreads();
        return v;
    }
};

#endif
