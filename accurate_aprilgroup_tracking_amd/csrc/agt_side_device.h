// agt_side_device.h -- device functions shared by the side libraries' kernels.  As in agt_device.h every section states the
// floating-point contraction it needs and the file ends with contraction off: a file that includes it re-states its own mode afterwards.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

// ---- the offline FP64 solves (agt_calib.hip, agt_camcal.hip): contracted, as those files' own arithmetic is
#pragma clang fp contract(fast)

// LDL^T of a symmetric positive definite 6 x 6 (upper triangle read), factored once and applied to several right-hand sides.
// The arithmetic of agt_solve6 with correctly rounded divisions: these are offline solves held to a numpy reference near FP64
// round-off, not links of a per-frame chain, so the reciprocal estimates of the pose solver buy nothing here.
struct AgtLdl6 { double L[6][6], iD[6]; };

__device__ __forceinline__ bool agt_ldl6_factor(const double A[36], AgtLdl6& F)
{
    double D[6];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
        double d = A[j * 6 + j];
#pragma unroll
        for (int k = 0; k < j; k++) d -= F.L[j][k] * F.L[j][k] * D[k];
        if (!(d > 0.0)) ok = false;
        D[j] = d;
        F.iD[j] = 1.0 / d;
#pragma unroll
        for (int i = j + 1; i < 6; i++) {
            double v = A[j * 6 + i];
#pragma unroll
            for (int k = 0; k < j; k++) v -= F.L[i][k] * F.L[j][k] * D[k];
            F.L[i][j] = v / d;
        }
    }
    return ok;
}

__device__ __forceinline__ void agt_ldl6_subst(const AgtLdl6& F, const double b[6], double x[6])
{
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double v = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) v -= F.L[i][k] * y[k];
        y[i] = v;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double v = y[i] * F.iD[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) v -= F.L[k][i] * x[k];
        x[i] = v;
    }
}

// The sum of one value per thread of a 1024-thread workgroup by a fixed tree: it is in part[0] (LDS, 1024 doubles) on return, behind a
// barrier.
__device__ __forceinline__ void agt_block_sum_1024(double acc, double* part)
{
    part[threadIdx.x] = acc;
    __syncthreads();
    for (int s = 512; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) part[threadIdx.x] += part[threadIdx.x + s];
        __syncthreads();
    }
}

// ---- the image stages (agt_tagcode.hip, agt_quadfit.hip, agt_quadfind.hip, agt_chess.hip): held to numpy statements operation by
// operation, nothing contracted
#pragma clang fp contract(off)

__device__ __forceinline__ bool agt_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (NaN fails)

// the bilinear blend of a 2 x 2 patch (i00 i10 / i01 i11) at the fractions (a, b), the four taps in this order
__device__ __forceinline__ double agt_blend4(double a, double b, double i00, double i10, double i01, double i11)
{
    return (1.0 - a) * (1.0 - b) * i00 + a * (1.0 - b) * i10 + (1.0 - a) * b * i01 + a * b * i11;
}

// that blend of the pixels (ix, iy) .. (ix + 1, iy + 1) of an 8-bit image; the caller has judged the point: all four addresses are formed
__device__ __forceinline__ double agt_bilinear_u8(const uint8_t* img, size_t pitch, int ix, int iy, double a, double b)
{
    const uint8_t* p = img + (size_t)iy * pitch + (size_t)ix;
    return agt_blend4(a, b, (double)p[0], (double)p[1], (double)p[pitch], (double)p[pitch + 1]);
}

// The sum of one value per lane in the order the headers state: P[l] = P[l] + P[l xor m] for m = TOP, TOP / 2 .. 1.  Every lane of an
// aligned group of 2 TOP lanes ends with the same bits: the whole wave by default, a 16-lane row for TOP = 8.
template <int TOP = 32>
__device__ __forceinline__ double agt_wave_sum_fixed(double v)
{
#pragma unroll
    for (int m = TOP; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}

// ---- ordered compaction: the kept elements of a frame get consecutive ids in element order, no workgroup waiting for another.  A
// workgroup owns a chunk, element  chunk * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x  in iteration it.  Three launches: the
// kept elements of every chunk (agt_chunk_total), one workgroup per frame turns the counts into exclusive prefixes, 256 chunks a round
// (agt_block_exclusive_sum), and every kept element reads its id off its chunk's prefix (agt_chunk_below, a barrier, agt_chunk_rank).
constexpr int AGT_SCAN_THREADS = 256, AGT_SCAN_ITERS = 4, AGT_SCAN_CHUNK = AGT_SCAN_THREADS * AGT_SCAN_ITERS;
constexpr int AGT_SCAN_WAVES = AGT_SCAN_THREADS / 64, AGT_SCAN_SEGS = AGT_SCAN_ITERS * AGT_SCAN_WAVES;

__device__ __forceinline__ int agt_wave_inclusive_sum(int v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int t = __shfl_up(v, d, 64);
        if (lane >= d) v += t;
    }
    return v;
}

// The exclusive sum of one value per thread over a 256-thread workgroup in thread order, and the workgroup's total.
// part: LDS, 4 ints; two barriers.
__device__ __forceinline__ int agt_block_exclusive_sum(int v, int* part, int& total)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int inc = agt_wave_inclusive_sum(v, lane);
    __syncthreads();                // (part may still be read from the round before)
    if (lane == 63) part[wave] = inc;
    __syncthreads();
    int before = 0;
    total = 0;
#pragma unroll
    for (int u = 0; u < 4; u++) { before += u < wave ? part[u] : 0; total += part[u]; }
    return before + inc - v;
}

// The chunk's total of what its waves counted (wave-uniform sums of ballot counts; T: int, or int2 for two counts at once).
// part: LDS, AGT_SCAN_WAVES values; one barrier.
template <class T>
__device__ __forceinline__ T agt_chunk_total(T wave_count, T* part)
{
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = wave_count;
    __syncthreads();
    T s = part[0];
#pragma unroll
    for (int v = 1; v < AGT_SCAN_WAVES; v++) s += part[v];
    return s;
}

// Iteration it of a chunk: the kept elements of this wave in lower lanes; the wave's count goes to seg (LDS, AGT_SCAN_SEGS ints).
__device__ __forceinline__ int agt_chunk_below(bool kept, int it, int* seg)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(kept);
    const int below = __popcll(m & ((1ull << lane) - 1ull));
    if (lane == 0) seg[it * AGT_SCAN_WAVES + (threadIdx.x >> 6)] = __popcll(m);
    return below;
}

// ... and, behind a barrier, the id of a kept element of iteration it: `first` is its chunk's exclusive prefix
__device__ __forceinline__ int agt_chunk_rank(int first, int below, int it, const int* seg)
{
    const int mine = it * AGT_SCAN_WAVES + (threadIdx.x >> 6);
    int id = first + below;
#pragma unroll
    for (int s = 0; s < AGT_SCAN_SEGS; s++) id += s < mine ? seg[s] : 0;
    return id;
}
