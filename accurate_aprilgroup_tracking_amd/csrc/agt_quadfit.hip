// libagt_quadfit.so (include/agt_quadfit.h): the edge refinement stage of a tag detector.  One translation unit, one kernel.
//
// quad_refine_kernel: one wave per quad, QUAD_WAVES waves per workgroup, no LDS, no atomics, the pass loop inside.
//   lane 16 e + i is station i of edge e: a 16-lane row is one edge
//   the station loop walks the 17 offsets with no divergent exit -- a sample point outside the frame is read at pixel (0, 0) instead
//   and the station is masked out of every sum afterwards
//   the station sums are xor butterflies inside a row (masks 8, 4, 2, 1: a fixed order, the same value in the 16 lanes of the row),
//   the used-station counts come out of one ballot, line e - 1 reaches row e by a shuffle from 48 lanes on, and the four new corners
//   are read back from lanes 0, 16, 32 and 48, so every lane starts the next pass with the whole quad.
// Every decision that ends a pass (station counts, the intersection's denominator) is taken on wave-uniform values or a ballot.
// Shared with the other image stages: the frame arguments and their rule (agt_side_frames.h), the fixed-order butterfly sum (here
// over a row: agt_wave_sum_fixed<8>) and the bilinear fetch (agt_side_device.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <stdint.h>

#include "agt_side_device.h"
#include "agt_side_frames.h"
#include "agt_side_math.h"
#include "../../include/agt_quadfit.h"

#pragma clang fp contract(off)

static_assert(AGT_QUADFIT_OK == agt_side::OK && AGT_QUADFIT_ERR_ARG == agt_side::ERR_ARG && AGT_QUADFIT_ERR_HIP == agt_side::ERR_HIP,
              "the codes of agt_side_math.h");

namespace {

using agt_side::Frames;

constexpr int QUAD_WAVES = 4;           // quads per workgroup
constexpr int MIN_USED = 8;             // used stations an edge needs

struct QuadCall {
    Frames F;
    int Q, total;
    const uint32_t* quads; const uint8_t* mask;
    double range; int iters; double min_strength;
    uint32_t* out32; double* out64; agt_quad_record* rec; uint8_t* ok; uint8_t* cmask;
};

// the sum over the 16 lanes of a row (masks 8, 4, 2, 1)
__device__ __forceinline__ double row_sum(double x) { return agt_wave_sum_fixed<8>(x); }

// corner j of four held in registers (no indexed private array: no scratch)
__device__ __forceinline__ double pick(const double (&v)[4], int j) { return j == 0 ? v[0] : j == 1 ? v[1] : j == 2 ? v[2] : v[3]; }

// +1 / -1: the common sign of the four cross products of consecutive edges; 0 when they are not of one sign or one is zero
__device__ __forceinline__ int convex_sign(const double (&x)[4], const double (&y)[4])
{
    bool pos = true, neg = true;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int j = (i + 1) & 3, k = (i + 2) & 3;
        const double cr = (x[j] - x[i]) * (y[k] - y[j]) - (y[j] - y[i]) * (x[k] - x[j]);
        pos = pos && cr > 0.0; neg = neg && cr < 0.0;
    }
    return pos ? 1 : neg ? -1 : 0;
}

// The bilinear sample at (x, y) when its 2 x 2 taps lie in the frame; otherwise `inside` is cleared and pixel (0, 0) .. (1, 1) is
// read: the address is formed from the judged, replaced integers only (width and height are at least 4).
__device__ __forceinline__ double sample(const uint8_t* __restrict__ img, size_t pitch, int w, int h, double x, double y, bool& inside)
{
    const double fx = floor(x), fy = floor(y);
    const bool in = fx >= 0.0 && fx <= (double)(w - 2) && fy >= 0.0 && fy <= (double)(h - 2);         // (NaN and inf fail)
    inside = inside && in;
    const int ix = in ? (int)fx : 0, iy = in ? (int)fy : 0;
    return agt_bilinear_u8(img, pitch, ix, iy, x - fx, y - fy);
}

__global__ __launch_bounds__(64 * QUAD_WAVES) void quad_refine_kernel(QuadCall C)
{
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * QUAD_WAVES + (threadIdx.x >> 6)));
    if (q >= C.total) return;
    const int b = q / C.Q;
    const int e = lane >> 4, i = lane & 15;

    // the input: kept as bits for the outputs of a refused quad, promoted for everything else
    uint32_t raw[8];
    double x[4], y[4];
#pragma unroll
    for (int j = 0; j < 8; j++) raw[j] = C.quads[(size_t)q * 8 + j];
#pragma unroll
    for (int j = 0; j < 4; j++) { x[j] = (double)__uint_as_float(raw[2 * j]); y[j] = (double)__uint_as_float(raw[2 * j + 1]); }

    int status = AGT_QUAD_OK, orient = 0;
    if (C.mask && C.mask[q] == 0) status = AGT_QUAD_MASKED;
    else {
        bool fin = true;
#pragma unroll
        for (int j = 0; j < 4; j++) fin = fin && fabs(x[j]) <= AGT_QUADFIT_MAX_COORD && fabs(y[j]) <= AGT_QUADFIT_MAX_COORD;     // (NaN and inf fail)
        orient = fin ? convex_sign(x, y) : 0;
        if (orient == 0) status = AGT_QUAD_DEGENERATE;
        else {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const double dx = x[(j + 1) & 3] - x[j], dy = y[(j + 1) & 3] - y[j];
                if (sqrt(dx * dx + dy * dy) < AGT_QUADFIT_MIN_EDGE) status = AGT_QUAD_SHORT;
            }
        }
    }

    int passes = 0;
    double strength = 0.0, shift = 0.0, resid = 0.0;
    double cx[4], cy[4];
#pragma unroll
    for (int j = 0; j < 4; j++) { cx[j] = x[j]; cy[j] = y[j]; }

    if (status == AGT_QUAD_OK) {
        double shoelace = 0.0;
#pragma unroll
        for (int j = 0; j < 4; j++) shoelace += x[j] * y[(j + 1) & 3] - x[(j + 1) & 3] * y[j];
        const double sg = shoelace > 0.0 ? 1.0 : -1.0;
        const uint8_t* img = C.F.p + (size_t)b * C.F.stride;
        const double u = (((double)i + 0.5) / 16.0 - 0.5) * 0.75;
        int refused = AGT_QUAD_OK;

        for (int pass = 0; pass < C.iters; pass++) {
            const double ax = pick(cx, e), ay = pick(cy, e), bx = pick(cx, (e + 1) & 3), by = pick(cy, (e + 1) & 3);
            const double dx = bx - ax, dy = by - ay;
            const double L = sqrt(dx * dx + dy * dy);
            const double nx = sg * dy / L, ny = sg * -dx / L;
            const double r = L / 8.0 < C.range ? L / 8.0 : C.range;
            const double px = ax + (u + 0.5) * dx, py = ay + (u + 0.5) * dy;
            bool inside = true;
            double Mc = 0.0, Mn = 0.0, gm = 0.0;
            for (int k = -8; k <= 8; k++) {
                const double o = r * (double)k / 8.0;
                const double I1 = sample(img, C.F.pitch, C.F.w, C.F.h, px + (o + 1.0) * nx, py + (o + 1.0) * ny, inside);
                const double I0 = sample(img, C.F.pitch, C.F.w, C.F.h, px + (o - 1.0) * nx, py + (o - 1.0) * ny, inside);
                const double dg = I1 - I0;
                if (dg > 0.0) {                 // (a dropped station's sums are never used)
                    Mc += dg * dg;
                    Mn += dg * dg * o;
                    gm = dg > gm ? dg : gm;
                }
            }
            const bool used = inside && Mc > 0.0;
            const double oi = used ? Mn / Mc : 0.0;
            const uint64_t ballot = __ballot(used);
            const int n0 = __popcll(ballot & 0xFFFFull), n1 = __popcll((ballot >> 16) & 0xFFFFull), n2 = __popcll((ballot >> 32) & 0xFFFFull),
                      n3 = __popcll(ballot >> 48);
            const double s0 = (double)(e == 0 ? n0 : e == 1 ? n1 : e == 2 ? n2 : n3);
            const double gsum = row_sum(used ? gm : 0.0);
            const double es = s0 > 0.0 ? gsum / s0 : 0.0;
            {
                const double e0 = __shfl(es, 0, 64), e1 = __shfl(es, 16, 64), e2 = __shfl(es, 32, 64), e3 = __shfl(es, 48, 64);
                const double m01 = e0 < e1 ? e0 : e1, m23 = e2 < e3 ? e2 : e3;
                strength = m01 < m23 ? m01 : m23;
            }
            if (n0 < MIN_USED || n1 < MIN_USED || n2 < MIN_USED || n3 < MIN_USED) { refused = AGT_QUAD_WEAK; break; }

            const double s1 = row_sum(used ? u : 0.0), s2 = row_sum(used ? u * u : 0.0), y0 = row_sum(oi), y1 = row_sum(used ? oi * u : 0.0);
            const double det = s0 * s2 - s1 * s1;
            const double alpha = (s2 * y0 - s1 * y1) / det, beta = (s0 * y1 - s1 * y0) / det;
            const double ee = used ? oi - (alpha + beta * u) : 0.0;
            const double er = sqrt(row_sum(ee * ee) / s0);
            {
                const double r0 = __shfl(er, 0, 64), r1 = __shfl(er, 16, 64), r2 = __shfl(er, 32, 64), r3 = __shfl(er, 48, 64);
                const double m01 = r0 > r1 ? r0 : r1, m23 = r2 > r3 ? r2 : r3;
                resid = m01 > m23 ? m01 : m23;
            }
            // line e about q_e, line e - 1 from the row before (48 lanes on, modulo the wave), also about q_e
            const double t0 = alpha - beta / 2.0, t1 = alpha + beta / 2.0;
            const double P0x = ax + t0 * nx, P0y = ay + t0 * ny, P1x = bx + t1 * nx, P1y = by + t1 * ny;
            const int src = (lane + 48) & 63;
            const double x1 = __shfl(P0x, src, 64) - ax, y1p = __shfl(P0y, src, 64) - ay, x2 = __shfl(P1x, src, 64) - ax, y2 = __shfl(P1y, src, 64) - ay;
            const double x3 = P0x - ax, y3 = P0y - ay, x4 = P1x - ax, y4 = P1y - ay;
            const double d0x = x2 - x1, d0y = y2 - y1p, d1x = x4 - x3, d1y = y4 - y3;
            const double den = d0x * d1y - d0y * d1x;
            const double l0 = sqrt(d0x * d0x + d0y * d0y), l1 = sqrt(d1x * d1x + d1y * d1y);
            if (__ballot(!(fabs(den) > 1e-12 * l0 * l1)) != 0ull) { refused = AGT_QUAD_DIVERGED; break; }
            const double c0 = x1 * y2 - y1p * x2, c1 = x3 * y4 - y3 * x4;
            const double X = ax + (d0x * c1 - c0 * d1x) / den, Y = ay + (d0y * c1 - c0 * d1y) / den;
#pragma unroll
            for (int j = 0; j < 4; j++) { cx[j] = __shfl(X, 16 * j, 64); cy[j] = __shfl(Y, 16 * j, 64); }
            passes++;
        }

        if (refused == AGT_QUAD_OK) {
            bool fin = true;
#pragma unroll
            for (int j = 0; j < 4; j++) fin = fin && agt_finite(cx[j]) && agt_finite(cy[j]);
            if (fin) {
#pragma unroll
                for (int j = 0; j < 4; j++) {
                    const double sx = cx[j] - x[j], sy = cy[j] - y[j];
                    const double s = sqrt(sx * sx + sy * sy);
                    shift = s > shift ? s : shift;
                }
            }
            if (!fin || convex_sign(cx, cy) != orient || shift > 2.0 * C.range) refused = AGT_QUAD_DIVERGED;
        }
        if (refused == AGT_QUAD_WEAK || strength < C.min_strength) status = AGT_QUAD_WEAK;
        else status = refused;
    }

    if (lane == 0) {
        agt_quad_record rec;
        rec.status = status; rec.passes = passes; rec.strength = strength; rec.shift = shift; rec.resid = resid;
        C.rec[q] = rec;
        const bool good = status == AGT_QUAD_OK;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            C.out32[(size_t)q * 8 + 2 * j] = good ? __float_as_uint((float)cx[j]) : raw[2 * j];
            C.out32[(size_t)q * 8 + 2 * j + 1] = good ? __float_as_uint((float)cy[j]) : raw[2 * j + 1];
        }
        if (C.out64) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                C.out64[(size_t)q * 8 + 2 * j] = good ? cx[j] : x[j];
                C.out64[(size_t)q * 8 + 2 * j + 1] = good ? cy[j] : y[j];
            }
        }
        const uint8_t ok = good ? 1 : 0;
        if (C.ok) C.ok[q] = ok;
        if (C.cmask) {
#pragma unroll
            for (int j = 0; j < 4; j++) C.cmask[(size_t)q * 4 + j] = ok;
        }
    }
}

}  // namespace

extern "C" {

int agt_quadfit_version(void) { return AGT_QUADFIT_VERSION; }

int agt_quad_refine(void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height, int B,
                    const float* d_quads, const uint8_t* d_mask, int Q, double range_px, int iters, double min_strength,
                    float* d_quads_out, double* d_quads64_out, agt_quad_record* d_records, uint8_t* d_ok, uint8_t* d_corner_mask)
{
    if (!agt_side::frames_ok(d_frames, pitch, frame_stride, width, height, 1, B, 4, AGT_QUADFIT_MAX_SIZE, AGT_QUADFIT_MAX_SIZE, INT_MAX)) return AGT_QUADFIT_ERR_ARG;
    if (!d_quads || !d_quads_out || !d_records) return AGT_QUADFIT_ERR_ARG;
    if (Q < 1 || (long long)B * (long long)Q > AGT_QUADFIT_MAX_QUADS) return AGT_QUADFIT_ERR_ARG;
    if (!(range_px > 0.0) || !(range_px <= AGT_QUADFIT_MAX_RANGE)) return AGT_QUADFIT_ERR_ARG;              // (NaN fails)
    if (iters < 1 || iters > AGT_QUADFIT_MAX_ITERS) return AGT_QUADFIT_ERR_ARG;
    if (!(min_strength >= 0.0) || !(min_strength <= 1.7976931348623157e308)) return AGT_QUADFIT_ERR_ARG;    // (NaN and inf fail)

    QuadCall C;
    C.F = Frames{ d_frames, pitch, frame_stride, width, height, B };
    C.Q = Q; C.total = B * Q;
    C.quads = reinterpret_cast<const uint32_t*>(d_quads); C.mask = d_mask;
    C.range = range_px; C.iters = iters; C.min_strength = min_strength;
    C.out32 = reinterpret_cast<uint32_t*>(d_quads_out); C.out64 = d_quads64_out; C.rec = d_records; C.ok = d_ok; C.cmask = d_corner_mask;
    hipLaunchKernelGGL(quad_refine_kernel, dim3(agt_side::div_up(C.total, QUAD_WAVES)), dim3(64 * QUAD_WAVES), 0, (hipStream_t)stream, C);
    if (hipGetLastError() != hipSuccess) return AGT_QUADFIT_ERR_HIP;
    return AGT_QUADFIT_OK;
}

}  // extern "C"
