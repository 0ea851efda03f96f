// Device only: PslLmGrid, the executor of lm_kernels.h (its contract is above psl_lm_levenberg) on a whole device, driven from the
// host, and the whole-device forms of the dense solve of gba_kernels.h.  A step is a plain stream-ordered launch on the context's
// stream; the order of the stream is the only synchronisation between steps.  No cooperative launch, no kernel that waits for
// another workgroup, no graph, no floating-point atomic.
//   par(n, f)    ceil(n / 256) workgroups of 256 threads, thread = index
//   one(f)       one thread
//   sum256(f)    one workgroup of 256 threads through psl_lm_reduce, then a read-back of one double
//   get(p)       a read-back of sizeof(*p) bytes behind a stream synchronisation
// A step's closure travels as the kernel argument, so it must hold what it needs by value (gba_kernels.h).  The first HIP error is
// kept in `err`; after it nothing more is launched and get / sum256 return 0, which ends the driver's loops.
#ifndef PSL_LM_GRID_H
#define PSL_LM_GRID_H

#include "gba_kernels.h"
#include "lm_device.h"

template <class Fn>
__global__ __launch_bounds__(PSL_LM_LANES) void k_lm_grid_par(int n, Fn f) {
    const int i = (int)(blockIdx.x * PSL_LM_LANES + threadIdx.x);
    if (i < n) f(i);
}
template <class Fn>
__global__ __launch_bounds__(1) void k_lm_grid_one(Fn f) {
    f();
}
template <class Fn>
__global__ __launch_bounds__(PSL_LM_LANES) void k_lm_grid_sum(Fn f, double* out) {
    __shared__ double s_red[2 * 4];
    int flip = 0;
    double v[1] = {f((int)threadIdx.x)};
    psl_lm_reduce<1, 1>(v, s_red, flip);
    if (threadIdx.x == 0) *out = v[0];
}

struct PslLmGrid {
    static constexpr bool tiled_solve = true;   // psl_gba_factor / _forward / _backward / _chain below are this executor's (gba_kernels.h)
    hipStream_t stream;
    double* d_sum;     // one double of HBM for sum256
    hipError_t err;
    long launches, readbacks;
    void note(hipError_t e) { if (err == hipSuccess) err = e; }
    template <class Fn> void par(int n, Fn f) {
        if (n <= 0 || err != hipSuccess) return;
        k_lm_grid_par<<<(unsigned)((n + PSL_LM_LANES - 1) / PSL_LM_LANES), PSL_LM_LANES, 0, stream>>>(n, f);
        ++launches;
        note(hipGetLastError());
    }
    template <class Fn> void one(Fn f) {
        if (err != hipSuccess) return;
        k_lm_grid_one<<<1, 1, 0, stream>>>(f);
        ++launches;
        note(hipGetLastError());
    }
    template <class V> V get(const V* p) {
        V v = V();
        if (err != hipSuccess) return v;
        note(hipMemcpyAsync(&v, p, sizeof(V), hipMemcpyDeviceToHost, stream));
        note(hipStreamSynchronize(stream));
        ++readbacks;
        return err == hipSuccess ? v : V();
    }
    template <class Fn> double sum256(Fn f) {
        if (err != hipSuccess) return 0.0;
        k_lm_grid_sum<<<1, PSL_LM_LANES, 0, stream>>>(f, d_sum);
        ++launches;
        note(hipGetLastError());
        return get(d_sum);
    }
};

// ---- the LDLt in column panels -----------------------------------------------------------------------------------------------------
// A panel is PSL_GRID_NB columns.  Every entry (i, j) of the panel belongs to one thread, which runs the entry's own subtraction
// chain in ascending k: first over the columns left of the panel (k < j0, tiles of L and of c[j][k] = L[j][k] D[k] staged through
// LDS, the product rounded as it is staged), then over the panel's own columns (j0 <= k < j).  Two launches per panel:
// k_grid_panel_diag (one workgroup: the panel's own rows, then the factorisation of the diagonal block in LDS) and
// k_grid_panel_rows (64 rows per workgroup below the panel: thread = row, its PSL_GRID_NB entries in registers).
#define PSL_GRID_NB 32
#define PSL_GRID_ROWS 64
#define PSL_GRID_CHUNK 512    // doubles of LDS that feed a chain of additions: two per thread, fetched into registers while the
                              // chain of the chunk before runs

__global__ __launch_bounds__(PSL_GRID_ROWS) void k_grid_panel_diag(double* S, double* Dd, int N, int j0, int nb, int32_t* ok) {
    __shared__ double Ls[PSL_GRID_NB][PSL_GRID_NB + 1];
    __shared__ double Ct[PSL_GRID_NB][PSL_GRID_NB + 2];   // [k][column]
    __shared__ double P[PSL_GRID_NB][PSL_GRID_NB + 1];
    __shared__ double Dp[PSL_GRID_NB], ccs[PSL_GRID_NB];
    const int t = threadIdx.x;
    const bool mine = t < nb;
    double acc[PSL_GRID_NB];
#pragma unroll
    for (int c = 0; c < PSL_GRID_NB; ++c) acc[c] = mine && c <= t ? S[(size_t)(j0 + c) * N + (j0 + t)] : 0.0;   // A[i][j] from the upper triangle
    for (int k0 = 0; k0 < j0; k0 += PSL_GRID_NB) {
        for (int idx = t; idx < PSL_GRID_NB * PSL_GRID_NB; idx += PSL_GRID_ROWS) {
            const int r = idx / PSL_GRID_NB, kk = idx % PSL_GRID_NB;
            const double v = r < nb ? S[(size_t)(j0 + r) * N + (k0 + kk)] : 0.0;
            Ls[r][kk] = v;
            Ct[kk][r] = v * Dd[k0 + kk];
        }
        __syncthreads();
        if (t < PSL_GRID_NB) {
#pragma unroll 2
            for (int kk = 0; kk < PSL_GRID_NB; ++kk) {
                const double l = Ls[t][kk];
#pragma unroll
                for (int c = 0; c < PSL_GRID_NB; ++c) acc[c] = acc[c] - l * Ct[kk][c];
            }
        }
        __syncthreads();
    }
    if (t < PSL_GRID_NB) {
#pragma unroll
        for (int c = 0; c < PSL_GRID_NB; ++c) P[t][c] = acc[c];
    }
    __syncthreads();
    for (int j = 0; j < nb; ++j) {   // uniform
        if (t < j) ccs[t] = P[j][t] * Dp[t];
        __syncthreads();
        double s = 0.0;
        if (t >= j && mine) {
            s = P[t][j];
            for (int k = 0; k < j; ++k) s = s - P[t][k] * ccs[k];
            if (t == j) {
                if (!(s > 0.0) || !(s <= PSL_LM_DBL_MAX)) *ok = 0;
                Dp[j] = s;
            }
        }
        __syncthreads();
        if (t > j && mine) P[t][j] = PSL_LM_DIV(s, Dp[j]);
        __syncthreads();
    }
    if (mine) {
        Dd[j0 + t] = Dp[t];
        for (int c = 0; c < t; ++c) S[(size_t)(j0 + t) * N + (j0 + c)] = P[t][c];
    }
}

__global__ __launch_bounds__(PSL_GRID_ROWS) void k_grid_panel_rows(double* S, const double* Dd, int N, int j0, int nb) {
    __shared__ double Ls[PSL_GRID_ROWS][PSL_GRID_NB + 1];
    __shared__ double Ct[PSL_GRID_NB][PSL_GRID_NB + 2];   // [k][column]; then the diagonal block as [j][k]
    __shared__ double dd[PSL_GRID_NB];
    const int t = threadIdx.x;
    const int i0 = j0 + nb + (int)blockIdx.x * PSL_GRID_ROWS, row = i0 + t;
    const bool mine = row < N;
    double acc[PSL_GRID_NB];
#pragma unroll
    for (int c = 0; c < PSL_GRID_NB; ++c) acc[c] = mine && c < nb ? S[(size_t)(j0 + c) * N + row] : 0.0;
    for (int k0 = 0; k0 < j0; k0 += PSL_GRID_NB) {
        for (int idx = t; idx < PSL_GRID_ROWS * PSL_GRID_NB; idx += PSL_GRID_ROWS) {
            const int r = idx / PSL_GRID_NB, kk = idx % PSL_GRID_NB;
            Ls[r][kk] = i0 + r < N ? S[(size_t)(i0 + r) * N + (k0 + kk)] : 0.0;
        }
        for (int idx = t; idx < PSL_GRID_NB * PSL_GRID_NB; idx += PSL_GRID_ROWS) {
            const int c = idx / PSL_GRID_NB, kk = idx % PSL_GRID_NB;
            Ct[kk][c] = c < nb ? S[(size_t)(j0 + c) * N + (k0 + kk)] * Dd[k0 + kk] : 0.0;
        }
        __syncthreads();
#pragma unroll 2
        for (int kk = 0; kk < PSL_GRID_NB; ++kk) {
            const double l = Ls[t][kk];
#pragma unroll
            for (int c = 0; c < PSL_GRID_NB; ++c) acc[c] = acc[c] - l * Ct[kk][c];
        }
        __syncthreads();
    }
    // the panel's own columns: c[j][k] = L[j][k] D[k] of the factored diagonal block
    for (int idx = t; idx < PSL_GRID_NB * PSL_GRID_NB; idx += PSL_GRID_ROWS) {
        const int j = idx / PSL_GRID_NB, k = idx % PSL_GRID_NB;
        Ct[j][k] = k < j && j < nb ? S[(size_t)(j0 + j) * N + (j0 + k)] * Dd[j0 + k] : 0.0;
    }
    if (t < PSL_GRID_NB) dd[t] = t < nb ? Dd[j0 + t] : 1.0;
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PSL_GRID_NB; ++j) {
        if (j < nb) {   // uniform
            double s = acc[j];
#pragma unroll
            for (int k = 0; k < j; ++k) s = s - acc[k] * Ct[j][k];
            acc[j] = PSL_LM_DIV(s, dd[j]);
        }
    }
    if (mine) {
#pragma unroll
        for (int c = 0; c < PSL_GRID_NB; ++c)
            if (c < nb) S[(size_t)row * N + (j0 + c)] = acc[c];
    }
}

static inline void psl_gba_factor(PslLmGrid& X, const PslGbaWs& G, int N) {
    for (int j0 = 0; j0 < N && X.err == hipSuccess; j0 += PSL_GRID_NB) {
        const int nb = N - j0 < PSL_GRID_NB ? N - j0 : PSL_GRID_NB;
        k_grid_panel_diag<<<1, PSL_GRID_ROWS, 0, X.stream>>>(G.B.S, G.B.Dd, N, j0, nb, G.B.flag);
        ++X.launches;
        const int below = N - j0 - nb;
        if (below > 0) {
            k_grid_panel_rows<<<(unsigned)((below + PSL_GRID_ROWS - 1) / PSL_GRID_ROWS), PSL_GRID_ROWS, 0, X.stream>>>(G.B.S, G.B.Dd, N, j0, nb);
            ++X.launches;
        }
        X.note(hipGetLastError());
    }
}

// ---- the forward substitution: rows in parallel behind a solved diagonal panel -----------------------------------------------------
// One launch per panel.  bs holds each row's running value; every workgroup solves the panel's nb rows itself (lane = row, the
// solved y[j] handed on by a shuffle, j ascending), workgroup 0 writes them to y, and every row below subtracts the panel's
// products in ascending k.  A row's value is read and written by its own thread alone.
__global__ __launch_bounds__(PSL_LM_LANES) void k_grid_forward(const double* S, double* bs, double* y, int N, int j0, int nb) {
    __shared__ double Ld[PSL_GRID_NB][PSL_GRID_NB + 1];
    __shared__ double Ys[PSL_GRID_NB];
    const int t = threadIdx.x;
    for (int idx = t; idx < PSL_GRID_NB * PSL_GRID_NB; idx += PSL_LM_LANES) {
        const int r = idx / PSL_GRID_NB, k = idx % PSL_GRID_NB;
        Ld[r][k] = k < r && r < nb ? S[(size_t)(j0 + r) * N + (j0 + k)] : 0.0;
    }
    __syncthreads();
    if (t < PSL_LM_GROUP) {   // the first wave
        double v = t < nb ? bs[j0 + t] : 0.0;
        for (int j = 0; j < nb; ++j) {   // uniform
            const double yj = __shfl(v, j, PSL_LM_GROUP);
            if (t > j && t < nb) v = v - Ld[t][j] * yj;
        }
        if (t < nb) {
            Ys[t] = v;
            if (blockIdx.x == 0) y[j0 + t] = v;
        }
    }
    __syncthreads();
    const int row = j0 + nb + (int)blockIdx.x * PSL_LM_LANES + t;
    if (row < N) {
        double s = bs[row];
        const double* L = S + (size_t)row * N + j0;
        for (int k = 0; k < nb; ++k) s = s - L[k] * Ys[k];
        bs[row] = s;
    }
}
static inline void psl_gba_forward(PslLmGrid& X, const PslGbaWs& G, int N) {
    for (int j0 = 0; j0 < N && X.err == hipSuccess; j0 += PSL_GRID_NB) {
        const int nb = N - j0 < PSL_GRID_NB ? N - j0 : PSL_GRID_NB;
        const int below = N - j0 - nb;
        const unsigned blocks = below > 0 ? (unsigned)((below + PSL_LM_LANES - 1) / PSL_LM_LANES) : 1u;
        k_grid_forward<<<blocks, PSL_LM_LANES, 0, X.stream>>>(G.B.S, G.B.bs, G.B.cc, N, j0, nb);
        ++X.launches;
        X.note(hipGetLastError());
    }
}

// ---- the backward substitution ------------------------------------------------------------------------------------------------------
// x[i]'s chain starts at k = i + 1, the value that arrives last, so the N - 1 - i subtractions of a row are serial behind x[i + 1]:
// N^2 / 2 dependent additions are the critical path.  One workgroup.  When x[k] is known all threads form its products
// L[k][i] x[k] (each rounded once) and store them at [i][k] of the upper triangle, which nothing reads after the factorisation;
// row i's products are then contiguous.  All threads fetch a chunk of them into registers (two doubles each) while one lane runs
// the chain of additions over the chunk before, which lies in LDS.
static_assert(PSL_GRID_CHUNK == 2 * PSL_LM_LANES, "a chunk is two doubles per thread");
// the two doubles of thread t in the chunk that starts at src[0] and has n <= PSL_GRID_CHUNK doubles
__device__ __forceinline__ void psl_grid_chunk_fetch(const double* src, int n, int t, double* v) {
    v[0] = t < n ? src[t] : 0.0;
    v[1] = t + PSL_LM_LANES < n ? src[t + PSL_LM_LANES] : 0.0;
}
// s - chunk (SUB) or s + chunk of the n doubles at src, chunk by chunk in ascending order; thread 0 returns the value.  Every
// thread of the workgroup calls it (it holds barriers).
template <bool SUB>
__device__ __forceinline__ double psl_grid_chain(const double* src, int n, double s, double* Ps) {
    const int t = threadIdx.x;
    double v[2];
    psl_grid_chunk_fetch(src, n < PSL_GRID_CHUNK ? n : PSL_GRID_CHUNK, t, v);
    for (int k0 = 0; k0 < n; k0 += PSL_GRID_CHUNK) {   // uniform
        const int m = n - k0 < PSL_GRID_CHUNK ? n - k0 : PSL_GRID_CHUNK;
        Ps[t] = v[0]; Ps[t + PSL_LM_LANES] = v[1];
        __syncthreads();
        const int rest = n - k0 - PSL_GRID_CHUNK;
        if (rest > 0) psl_grid_chunk_fetch(src + k0 + PSL_GRID_CHUNK, rest < PSL_GRID_CHUNK ? rest : PSL_GRID_CHUNK, t, v);
        if (t == 0)
            for (int idx = 0; idx < m; ++idx) s = SUB ? s - Ps[idx] : s + Ps[idx];
        __syncthreads();
    }
    return s;
}
__global__ __launch_bounds__(PSL_LM_LANES) void k_grid_backward(double* S, const double* y, const double* Dd, double* x, int N) {
    __shared__ double Ps[PSL_GRID_CHUNK];
    __shared__ double s_x;
    const int t = threadIdx.x;
    for (int i = N - 1; i >= 0; --i) {   // uniform
        double s = 0.0;
        if (t == 0) s = PSL_LM_DIV(y[i], Dd[i]);
        s = psl_grid_chain<true>(S + (size_t)i * N + (i + 1), N - 1 - i, s, Ps);
        if (t == 0) { x[i] = s; s_x = s; }
        __syncthreads();
        const double xi = s_x;
        for (int r = t; r < i; r += PSL_LM_LANES) S[(size_t)r * N + i] = S[(size_t)i * N + r] * xi;
        __syncthreads();   // the products are visible to the workgroup before the next row fetches them
    }
}
static inline void psl_gba_backward(PslLmGrid& X, const PslGbaWs& G, int N) {
    if (X.err != hipSuccess || N <= 0) return;
    k_grid_backward<<<1, PSL_LM_LANES, 0, X.stream>>>(G.B.S, G.B.cc, G.B.Dd, G.B.xp, N);
    ++X.launches;
    X.note(hipGetLastError());
}

// ---- one chain of additions over a dense buffer: all threads stage a chunk into LDS, one lane adds ----------------------------------
__global__ __launch_bounds__(PSL_LM_LANES) void k_grid_chain(const double* buf, int n, double* out) {
    __shared__ double Ps[PSL_GRID_CHUNK];
    const double s = psl_grid_chain<false>(buf, n, 0.0, Ps);
    if (threadIdx.x == 0) *out = s;
}
static inline void psl_gba_chain(PslLmGrid& X, const PslGbaWs&, const double* buf, int n, double* out) {
    if (X.err != hipSuccess) return;
    k_grid_chain<<<1, PSL_LM_LANES, 0, X.stream>>>(buf, n, out);
    ++X.launches;
    X.note(hipGetLastError());
}

#endif
