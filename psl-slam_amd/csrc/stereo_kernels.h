// HIP kernels of the stereo Frame constructor (gfx950, wave64): Frame::ComputeStereoMatches src/Frame.cc:1165-1340 on
// rectified pairs.  Product code.  The reference semantics each step reproduces are listed at
// pslfe_frame_set_from_orb_stereo in include/pslfe.h.
//
//   k_stereo_rows    one workgroup per pair: the right keypoints binned by their own level-0 row (count, scan, fill; CSR of
//                    16-bit indices).  A left keypoint's candidates lie in the rows within `band` of its own, one contiguous run.
//   k_stereo_match   one wave per left keypoint: the row-band / octave / disparity gates and the Hamming distance with lanes
//                    over the candidates, the least (dist, iR) by a wave reduction; then the 11 x 11 x 11 SAD sweep with lanes
//                    over (incR, row), the parabola fit and the rescale.  Integer SAD: every value is below 2^24, so the
//                    reference's float arithmetic on them is exact.
//   k_stereo_filter  one workgroup per pair: the median SAD of the accepted keypoints by a two-pass 8-bit histogram select in
//                    LDS (SAD <= 121 * 510 < 2^16; each pass's bin found by a block prefix sum), then the 1.5 * 1.4 * median threshold.
#ifndef PSL_STEREO_KERNELS_H
#define PSL_STEREO_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/pslfe.h"
#include "psl_device_math.h"

#define PSL_ST_W 5            // w = L = 5 (src/Frame.cc:1261, :1268)
#define PSL_ST_TH_ORB 75      // thOrbDist = (TH_HIGH + TH_LOW) / 2
#define PSL_ST_TH_HIGH 100    // ORBmatcher::TH_HIGH, the initial bestDist (:1221)
#define PSL_ST_MAX_ROWS 4096  // level-0 rows (the extractor's limit)
#define PSL_ST_KPW 4          // left keypoints per wave of k_stereo_match

struct StereoPyr {  // mvImagePyramid of one handle: level 0 of frame f at img0 + f*fstride0, level l >= 1 at pyr + f*pyr_fstride + off[l]
    const uint8_t* img0;
    size_t fstride0;
    const uint8_t* pyr;
    size_t pyr_fstride;
    int w[PSLFE_MAX_LEVELS], h[PSLFE_MAX_LEVELS], pitch[PSLFE_MAX_LEVELS];
    size_t off[PSLFE_MAX_LEVELS];
};

struct StereoArgs {
    // result arrays of the two extractors, at the pair's first frame (left0 / right0); pair p = frame p of these
    const PslKeyPoint* kpsL;
    const uint8_t* descL;
    const int* cntL;
    int capL, left0;
    const PslKeyPoint* kpsR;
    const uint8_t* descR;
    const int* cntR;
    int capR, right0;
    StereoPyr PL, PR;
    float scale[PSLFE_MAX_LEVELS], inv_scale[PSLFE_MAX_LEVELS];
    int nlevels, rows, band;  // rows: level-0 image rows; band: rows scanned on either side of a left keypoint's row
    float maxD, bf;
    int* rowstart;            // [pair][rows + 1]
    uint16_t* rowidx;         // [pair][capR]
    // outputs, slot slot0 + p at [(slot0 + p) * cap]
    float* uright;
    float* depth;
    int32_t* tidx;
    int32_t* tsad;
    int slot0, cap;
};

__device__ __forceinline__ const uint8_t* psl_st_level(const StereoPyr& P, int level, int frame) {
    return level == 0 ? P.img0 + (size_t)frame * P.fstride0 : P.pyr + (size_t)frame * P.pyr_fstride + P.off[level];
}

// row bin of a right keypoint: (int)y inside the image, clamped to the first / last row outside it (NaN -> 0).  Whether a keypoint
// is a candidate is decided by the exact band test; the bin only has to put every candidate inside the scanned rows.
__device__ __forceinline__ int psl_st_bin(float y, int rows) {
    return y >= 0.f ? (y < (float)rows ? (int)y : rows - 1) : 0;
}

// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(1024) void k_stereo_rows(StereoArgs A) {
    __shared__ int s_cnt[PSL_ST_MAX_ROWS];
    __shared__ int s_w[17];
    const int p = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, rows = A.rows;
    const int nR = min(A.cntR[p], A.capR);
    const PslKeyPoint* kR = A.kpsR + (size_t)p * A.capR;
    int* rs = A.rowstart + (size_t)p * (rows + 1);
    uint16_t* ri = A.rowidx + (size_t)p * A.capR;
    for (int r = tid; r < rows; r += 1024) s_cnt[r] = 0;
    __syncthreads();
    for (int i = tid; i < nR; i += 1024) atomicAdd(&s_cnt[psl_st_bin(kR[i].y, rows)], 1);
    __syncthreads();
    // exclusive scan, four rows per thread (rows <= 4096)
    const int c0 = tid * 4;
    int v[4], mine = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) { v[k] = c0 + k < rows ? s_cnt[c0 + k] : 0; mine += v[k]; }
    int inc = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    if (tid == 0) {
        int acc = 0;
        for (int k = 0; k < 16; ++k) { const int t = s_w[k]; s_w[k] = acc; acc += t; }
        s_w[16] = acc;
    }
    __syncthreads();
    int st = inc - mine + s_w[wave];
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (c0 + k < rows) { rs[c0 + k] = st; s_cnt[c0 + k] = st; st += v[k]; }   // row start, then the row's fill cursor
    if (tid == 0) rs[rows] = s_w[16];
    __syncthreads();
    for (int i = tid; i < nR; i += 1024) ri[atomicAdd(&s_cnt[psl_st_bin(kR[i].y, rows)], 1)] = (uint16_t)i;
}

// ---------------------------------------------------------------------------------------------
// grid (ceil(capL / (4 * PSL_ST_KPW)), npairs), 256 threads.  Every branch below depends on the wave's keypoint only (or on
// values reduced over the wave), so the shuffles run with all 64 lanes.
__global__ __launch_bounds__(256) void k_stereo_match(StereoArgs A) {
    const int p = blockIdx.y, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int nL = min(min(A.cntL[p], A.capL), A.cap);
    const PslKeyPoint* kL = A.kpsL + (size_t)p * A.capL;
    const PslKeyPoint* kR = A.kpsR + (size_t)p * A.capR;
    const uint32_t* dL = reinterpret_cast<const uint32_t*>(A.descL + (size_t)p * A.capL * 32);
    const uint32_t* dR = reinterpret_cast<const uint32_t*>(A.descR + (size_t)p * A.capR * 32);
    const int* rs = A.rowstart + (size_t)p * (A.rows + 1);
    const uint16_t* ri = A.rowidx + (size_t)p * A.capR;
    const size_t obase = (size_t)(A.slot0 + p) * A.cap;
    for (int k = 0; k < PSL_ST_KPW; ++k) {
        const int i = (blockIdx.x * 4 + wave) * PSL_ST_KPW + k;
        if (i >= nL) break;
        const PslKeyPoint kp = kL[i];
        const float uL = kp.x, vL = kp.y;
        const int oL = kp.octave;
        int out_idx = -1, out_sad = -1;
        float out_ur = -1.f, out_dep = -1.f;
        // vRowIndices[vL]: a row outside the image has no candidates (convention)
        bool go = vL >= 0.f && vL < (float)A.rows && oL >= 0 && oL < A.nlevels;
        const int row = go ? (int)vL : 0;
        const float minU = PSL_FSUB(uL, A.maxD), maxU = PSL_FSUB(uL, 0.0f);   // minD = 0
        if (maxU < 0.f) go = false;
        uint32_t best = 0xffffffffu;
        if (go) {
            uint32_t qd[8];
#pragma unroll
            for (int w = 0; w < 8; ++w) qd[w] = dL[(size_t)i * 8 + w];
            const int j0 = rs[max(row - A.band, 0)], j1 = rs[min(row + A.band, A.rows - 1) + 1];
            for (int j = j0 + lane; j < j1; j += 64) {
                const int iR = ri[j];
                const PslKeyPoint R = kR[iR];
                if (R.octave < 0 || R.octave >= A.nlevels) continue;
                const float r = PSL_FMUL(2.0f, A.scale[R.octave]);                        // :1186
                const int maxr = (int)__builtin_ceilf(PSL_FADD(R.y, r)), minr = (int)__builtin_floorf(PSL_FSUB(R.y, r));
                if (row < minr || row > maxr) continue;
                if (R.octave < oL - 1 || R.octave > oL + 1) continue;                      // :1232
                if (!(R.x >= minU && R.x <= maxU)) continue;                               // :1237
                const uint32_t dist = (uint32_t)psl_hamming256(qd, dR + (size_t)iR * 8);
                if (dist < PSL_ST_TH_HIGH) best = min(best, (dist << 16) | (uint32_t)iR);
            }
        }
        best = psl_wave_min_u32(best);
        if (go && best != 0xffffffffu && (int)(best >> 16) < PSL_ST_TH_ORB) {
            const int iR = (int)(best & 0xffffu);
            out_idx = iR;
            const float s = A.inv_scale[oL];
            const float suL = __builtin_roundf(PSL_FMUL(uL, s)), svL = __builtin_roundf(PSL_FMUL(vL, s));
            const float sR0 = __builtin_roundf(PSL_FMUL(kR[iR].x, s));
            const float iniu = PSL_FSUB(PSL_FADD(sR0, (float)PSL_ST_W), (float)PSL_ST_W);    // scaleduR0+L-w (:1270)
            const float endu = PSL_FADD(PSL_FADD(PSL_FADD(sR0, (float)PSL_ST_W), (float)PSL_ST_W), 1.0f);
            const int colsL = A.PL.w[oL], rowsL = A.PL.h[oL], colsR = A.PR.w[oL], rowsR = A.PR.h[oL];
            bool ok = !(iniu < 0.f || endu >= (float)colsR);
            // both windows inside the level images (convention; always so for keypoints of the extractor)
            ok = ok && svL >= 5.f && svL + 5.f < (float)min(rowsL, rowsR) && suL >= 5.f && suL + 5.f < (float)colsL && sR0 >= 10.f &&
                 sR0 + 10.f < (float)colsR;
            if (ok) {
                const int y0 = (int)svL, xl = (int)suL, xr = (int)sR0;
                const int pitchL = A.PL.pitch[oL], pitchR = A.PR.pitch[oL];
                const uint8_t* IL = psl_st_level(A.PL, oL, A.left0 + p) + (size_t)y0 * pitchL + xl;
                const uint8_t* IR = psl_st_level(A.PR, oL, A.right0 + p) + (size_t)y0 * pitchR + xr;
                const int cL = IL[0];
                int part[2];
#pragma unroll
                for (int hh = 0; hh < 2; ++hh) {   // lane t = (incR + 5) * 11 + (row + 5): one row of one window offset
                    const int t = lane + 64 * hh;
                    int sum = 0;
                    if (t < 121) {
                        const int incR = t / 11 - PSL_ST_W, rr = t % 11 - PSL_ST_W;
                        const int cR = IR[incR];
                        const uint8_t* pl = IL + (ptrdiff_t)rr * pitchL - PSL_ST_W;
                        const uint8_t* pr = IR + (ptrdiff_t)rr * pitchR + incR - PSL_ST_W;
#pragma unroll
                        for (int c = 0; c < 11; ++c) sum += abs(((int)pl[c] - cL) - ((int)pr[c] - cR));
                    }
                    part[hh] = sum;
                }
                // vDists[incR + 5] on lane incR + 5
                const int li = lane < 11 ? lane : 0;
                int D = 0;
#pragma unroll
                for (int r = 0; r < 11; ++r) {
                    const int t = li * 11 + r;
                    const int a = __shfl(part[0], t & 63), b = __shfl(part[1], (t - 64) & 63);
                    D += t < 64 ? a : b;
                }
                const uint32_t m = psl_wave_min_u32(lane < 11 ? ((uint32_t)D << 4) | (uint32_t)lane : 0xffffffffu);   // first minimum
                const int binc = (int)(m & 15u), d2i = (int)(m >> 4);
                const int d1i = __shfl(D, max(binc - 1, 0)), d3i = __shfl(D, min(binc + 1, 10));
                if (binc != 0 && binc != 2 * PSL_ST_W) {                                     // bestincR == +-L (:1293)
                    const float d1 = (float)d1i, d2 = (float)d2i, d3 = (float)d3i;
                    const float deltaR = PSL_FDIV(PSL_FSUB(d1, d3), PSL_FMUL(2.0f, PSL_FSUB(PSL_FADD(d1, d3), PSL_FMUL(2.0f, d2))));
                    if (!(deltaR < -1.f || deltaR > 1.f)) {
                        float bestuR = PSL_FMUL(A.scale[oL], PSL_FADD(PSL_FADD(sR0, (float)(binc - PSL_ST_W)), deltaR));
                        float disparity = PSL_FSUB(uL, bestuR);
                        if (disparity >= 0.f && disparity < A.maxD) {
                            if (disparity <= 0.f) {
                                disparity = 0.01f;
                                bestuR = (float)PSL_DSUB((double)uL, 0.01);
                            }
                            out_dep = PSL_FDIV(A.bf, disparity);
                            out_ur = bestuR;
                            out_sad = d2i;
                        }
                    }
                }
            }
        }
        if (lane == 0) {
            A.uright[obase + i] = out_ur;
            A.depth[obase + i] = out_dep;
            A.tidx[obase + i] = out_idx;
            A.tsad[obase + i] = out_sad;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// For 256 threads: the bin holding the k-th smallest (from 0) of the values counted in the 256-bin LDS histogram s_h (more than k
// of them), and k's rank inside that bin, by a block-wide prefix sum with one bin per thread; the one thread whose bin spans rank k
// writes *s_bin / *s_rank.  Ends with a barrier, so every thread may read them.
__device__ __forceinline__ void psl_st_select(const int* s_h, int k, int* s_w, int* s_bin, int* s_rank) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int c = s_h[tid];
    int inc = c;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) { const int u = __shfl_up(inc, o); if (lane >= o) inc += u; }
    if (lane == 63) s_w[wave] = inc;
    __syncthreads();
    for (int w = 0; w < wave; ++w) inc += s_w[w];
    const int excl = inc - c;
    if (excl <= k && k < inc) { *s_bin = tid; *s_rank = k - excl; }
    __syncthreads();
}

__global__ __launch_bounds__(256) void k_stereo_filter(StereoArgs A) {
    __shared__ int s_h[256];
    __shared__ int s_w[4];
    __shared__ int s_m, s_sel, s_rank;
    const int p = blockIdx.x, tid = threadIdx.x;
    const int n = min(min(A.cntL[p], A.capL), A.cap);
    const size_t obase = (size_t)(A.slot0 + p) * A.cap;
    const int32_t* sad = A.tsad + obase;
    s_h[tid] = 0;
    if (tid == 0) s_m = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int v = sad[i];
        if (v >= 0) { atomicAdd(&s_h[v >> 8], 1); atomicAdd(&s_m, 1); }
    }
    __syncthreads();
    const int M = s_m;
    if (M == 0) return;   // nothing accepted: nothing filtered (convention)
    psl_st_select(s_h, M / 2, s_w, &s_sel, &s_rank);   // high byte of the (M/2)-th smallest
    const int hi = s_sel, rank = s_rank;
    s_h[tid] = 0;
    __syncthreads();
    for (int i = tid; i < n; i += 256) {
        const int v = sad[i];
        if (v >= 0 && (v >> 8) == hi) atomicAdd(&s_h[v & 255], 1);
    }
    __syncthreads();
    psl_st_select(s_h, rank, s_w, &s_sel, &s_rank);     // its low byte
    const float median = (float)((hi << 8) | s_sel);
    const float thDist = PSL_FMUL(PSL_FMUL(1.5f, 1.4f), median);
    for (int i = tid; i < n; i += 256) {
        const int v = sad[i];
        if (v >= 0 && !((float)v < thDist)) { A.uright[obase + i] = -1.f; A.depth[obase + i] = -1.f; }
    }
}

#endif
