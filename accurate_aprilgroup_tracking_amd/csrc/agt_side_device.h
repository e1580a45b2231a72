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

// ---- the detector stages (agt_tagcode.hip, agt_quadfit.hip): held to numpy statements operation by operation, nothing contracted
#pragma clang fp contract(off)

__device__ __forceinline__ bool agt_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }      // (NaN fails)

// the bilinear blend of a 2 x 2 patch (i00 i10 / i01 i11) at the fractions (a, b), the four taps in this order
__device__ __forceinline__ double agt_blend4(double a, double b, double i00, double i10, double i01, double i11)
{
    return (1.0 - a) * (1.0 - b) * i00 + a * (1.0 - b) * i10 + (1.0 - a) * b * i01 + a * b * i11;
}
