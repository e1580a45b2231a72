// libagt_draw.so (include/agt_draw.h): the output stage -- display lists painted into frames in HBM.  One translation unit, two kernels.
//
// draw_raster_kernel: a workgroup of TILE_W x TILE_H threads owns a tile of as many pixels, one pixel per thread (gather, not scatter).
//   The list is taken in chunks of AGT_DRAW_CHUNK = the workgroup's size, LAST chunk first: thread t judges primitive base + t (validity,
//   then bounding box against the tile), a ballot and the earlier waves' counts give the survivor its place in LDS in list order.  Every
//   pixel that has not been hit yet walks the chunk's survivors from the last to the first; the first hit is the primitive that shows.
//   Every barrier sits in wave-uniform control flow (the chunk loop's bounds are the kernel's arguments).  A pixel is written once, by its
//   own thread, after the last chunk; a pixel outside the frame belongs to no thread that forms an address.
// draw_pose_lists_kernel: one thread per point; it writes the point's dot and the outline segment that starts at it.
// Shared with the other image stages: the frame arguments (here written to: MutableFrames) and their rule (agt_side_frames.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <stdint.h>

#include "agt_side_frames.h"
#include "agt_side_math.h"
#include "../../include/agt_draw.h"

static_assert(AGT_DRAW_OK == agt_side::OK && AGT_DRAW_ERR_ARG == agt_side::ERR_ARG && AGT_DRAW_ERR_HIP == agt_side::ERR_HIP,
              "the codes of agt_side_math.h");

namespace {

using agt_side::div_up;

constexpr int TILE_W = 32, TILE_H = 8;
constexpr int THREADS = TILE_W * TILE_H;
constexpr int WAVES = THREADS / 64;
constexpr int MAX_BATCH_Z = 65535;          // frames per launch (the grid's z extent)
static_assert(THREADS == AGT_DRAW_CHUNK, "a chunk is one primitive per thread");
static_assert(sizeof(agt_draw_prim) == 32, "agt_draw_prim is 32 bytes");

struct RasterCall {
    agt_side::MutableFrames F;
    int channels, P;
    const agt_draw_prim* prims;
    unsigned flags;
};

// what a pixel needs of a surviving primitive
struct Survivor { int kind, x0, y0, x1, y1, size; uint32_t color; int pad; };

__device__ __forceinline__ bool coord_ok(int v) { return v >= -AGT_DRAW_MAX_COORD && v <= AGT_DRAW_MAX_COORD; }

// does primitive s cover pixel (px, py)?  s is valid: |coordinates| <= 32767, 0 <= size <= 64; 0 <= px, py < 16384
__device__ __forceinline__ bool covers(const Survivor& s, int px, int py)
{
    const long long ax = px - s.x0, ay = py - s.y0;                 // p - a
    if (s.kind == AGT_DRAW_DISC) {
        const long long r = s.size;
        return ax * ax + ay * ay <= r * r + r;
    }
    const long long dx = s.x1 - s.x0, dy = s.y1 - s.y0;
    const long long T2 = (long long)s.size * s.size;
    const long long L2 = dx * dx + dy * dy;                         // < 2^34
    const long long t = ax * dx + ay * dy;                          // |t| < 2^34
    if (t <= 0) return 4 * (ax * ax + ay * ay) <= T2;
    if (t >= L2) {
        const long long bx = px - s.x1, by = py - s.y1;
        return 4 * (bx * bx + by * by) <= T2;
    }
    long long cr = dx * ay - dy * ax;                               // |cr| < 2^34: its square need not fit
    cr = cr < 0 ? -cr : cr;
    if (cr > (1ll << 22)) return false;                             // 4 cr^2 > 2^46 > T2 L2
    return 4 * cr * cr <= T2 * L2;
}

__global__ __launch_bounds__(THREADS) void draw_raster_kernel(RasterCall C, int batch0)
{
    __shared__ Survivor s_list[AGT_DRAW_CHUNK];
    __shared__ int s_count[WAVES];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int tx0 = blockIdx.x * TILE_W, ty0 = blockIdx.y * TILE_H;
    const int tx1 = tx0 + TILE_W - 1, ty1 = ty0 + TILE_H - 1;       // the tile, inclusive (it may reach past the frame)
    const int b = batch0 + blockIdx.z;
    const int px = tx0 + (tid & (TILE_W - 1)), py = ty0 + tid / TILE_W;
    const bool inside = px < C.F.w && py < C.F.h;

    bool done = !inside, hit = false;
    uint32_t color = 0;

    const int chunks = (C.P + AGT_DRAW_CHUNK - 1) / AGT_DRAW_CHUNK;
    for (int c = chunks - 1; c >= 0; c--) {
        const int idx = c * AGT_DRAW_CHUNK + tid;
        Survivor s = {AGT_DRAW_NONE, 0, 0, 0, 0, 0, 0u, 0};
        bool keep = false;
        if (idx < C.P) {
            const agt_draw_prim p = C.prims[(size_t)b * C.P + idx];
            const bool valid = (p.kind == AGT_DRAW_DISC || p.kind == AGT_DRAW_SEGMENT) && coord_ok(p.x0) && coord_ok(p.y0) && coord_ok(p.x1)
                               && coord_ok(p.y1) && p.size >= 0 && p.size <= AGT_DRAW_MAX_SIZE;
            if (valid) {
                // bounding box: a disc reaches `size` from its centre, a segment (size + 1) / 2 >= T / 2 from its two ends' box
                const bool disc = p.kind == AGT_DRAW_DISC;
                const int m = disc ? p.size : (p.size + 1) / 2;
                const int x1 = disc ? p.x0 : p.x1, y1 = disc ? p.y0 : p.y1;
                const int lox = (p.x0 < x1 ? p.x0 : x1) - m, hix = (p.x0 < x1 ? x1 : p.x0) + m;
                const int loy = (p.y0 < y1 ? p.y0 : y1) - m, hiy = (p.y0 < y1 ? y1 : p.y0) + m;
                keep = lox <= tx1 && hix >= tx0 && loy <= ty1 && hiy >= ty0;
                s.kind = p.kind; s.x0 = p.x0; s.y0 = p.y0; s.x1 = p.x1; s.y1 = p.y1; s.size = p.size;
                s.color = (uint32_t)p.color[0] | ((uint32_t)p.color[1] << 8) | ((uint32_t)p.color[2] << 16);
            }
        }
        const uint64_t mask = __ballot(keep);
        if (lane == 0) s_count[wave] = __popcll(mask);
        __syncthreads();
        int before = 0, count = 0;
#pragma unroll
        for (int v = 0; v < WAVES; v++) {
            const int n = s_count[v];
            before += v < wave ? n : 0;
            count += n;
        }
        if (keep) s_list[before + __popcll(mask & ((1ull << lane) - 1ull))] = s;
        __syncthreads();
        if (!done) {
            for (int k = count - 1; k >= 0; k--) {
                const Survivor q = s_list[k];
                if (covers(q, px, py)) { color = q.color; hit = true; done = true; break; }
            }
        }
        __syncthreads();            // the next chunk overwrites s_list and s_count
    }

    if (!inside || !(hit || (C.flags & AGT_DRAW_CLEAR))) return;
    uint8_t* out = C.F.p + (size_t)b * C.F.stride + (size_t)py * C.F.pitch + (size_t)px * (size_t)C.channels;
    out[0] = (uint8_t)(color & 0xFFu);
    if (C.channels == 3) {
        out[1] = (uint8_t)((color >> 8) & 0xFFu);
        out[2] = (uint8_t)((color >> 16) & 0xFFu);
    }
}

struct ListCall {
    const void* points; int f64, n, total;
    const double* gate; size_t gate_stride;
    int w, h, radius, thickness;
    uint32_t dot_color, line_color;
    agt_draw_prim* dots; agt_draw_prim* outline;
};

__device__ __forceinline__ double point_coord(const ListCall& C, size_t i)
{
    return C.f64 ? static_cast<const double*>(C.points)[i] : (double)static_cast<const float*>(C.points)[i];
}

__device__ __forceinline__ bool finite64(double v) { return fabs(v) <= 1.7976931348623157e308; }       // (NaN fails)

// v (already rounded or truncated to an integer value) names a pixel of [0, limit)
__device__ __forceinline__ bool in_range(double v, int limit) { return v >= 0.0 && v < (double)limit; }

__device__ __forceinline__ agt_draw_prim make_prim(int kind, int x0, int y0, int x1, int y1, int size, uint32_t color)
{
    agt_draw_prim p;
    p.kind = kind; p.x0 = x0; p.y0 = y0; p.x1 = x1; p.y1 = y1; p.size = size;
    p.color[0] = (uint8_t)(color & 0xFFu); p.color[1] = (uint8_t)((color >> 8) & 0xFFu); p.color[2] = (uint8_t)((color >> 16) & 0xFFu); p.color[3] = 0;
    p.reserved = 0;
    return p;
}

__global__ __launch_bounds__(256) void draw_pose_lists_kernel(ListCall C)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= C.total) return;
    const int b = i / C.n;
    const agt_draw_prim none = make_prim(AGT_DRAW_NONE, 0, 0, 0, 0, 0, 0u);
    agt_draw_prim dot = none, seg = none;
    const bool drawn = !C.gate || C.gate[(size_t)b * C.gate_stride] == 1.0;     // (NaN fails)
    if (drawn) {
        const double x = point_coord(C, 2 * (size_t)i), y = point_coord(C, 2 * (size_t)i + 1);
        if (finite64(x) && finite64(y)) {
            const double rx = rint(x), ry = rint(y);                            // half to even
            if (in_range(rx, C.w) && in_range(ry, C.h)) dot = make_prim(AGT_DRAW_DISC, (int)rx, (int)ry, (int)rx, (int)ry, C.radius, C.dot_color);
        }
        // the outline segment from this corner to the next of its group of four, if all four are in the frame
        const int g0 = i & ~3, j = i & 3;
        bool all_in = true;
        int qx[4], qy[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
            const double u = point_coord(C, 2 * (size_t)(g0 + k)), v = point_coord(C, 2 * (size_t)(g0 + k) + 1);
            const bool fin = finite64(u) && finite64(v);
            const double tu = fin ? trunc(u) : -1.0, tv = fin ? trunc(v) : -1.0;
            const bool in = in_range(tu, C.w) && in_range(tv, C.h);
            all_in = all_in && in;
            qx[k] = in ? (int)tu : 0; qy[k] = in ? (int)tv : 0;
        }
        if (all_in) {
            const int ax = j == 0 ? qx[0] : j == 1 ? qx[1] : j == 2 ? qx[2] : qx[3], ay = j == 0 ? qy[0] : j == 1 ? qy[1] : j == 2 ? qy[2] : qy[3];
            const int bx = j == 0 ? qx[1] : j == 1 ? qx[2] : j == 2 ? qx[3] : qx[0], by = j == 0 ? qy[1] : j == 1 ? qy[2] : j == 2 ? qy[3] : qy[0];
            seg = make_prim(AGT_DRAW_SEGMENT, ax, ay, bx, by, C.thickness, C.line_color);
        }
    }
    C.dots[i] = dot;
    C.outline[i] = seg;
}

}  // namespace

extern "C" {

int agt_draw_version(void) { return AGT_DRAW_VERSION; }

int agt_draw_raster(void* stream, uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height, int channels, int B,
                    const agt_draw_prim* d_prims, int P, unsigned flags)
{
    if (channels != 1 && channels != 3) return AGT_DRAW_ERR_ARG;
    if (!agt_side::frames_ok(d_frames, pitch, frame_stride, width, height, channels, B, 1, AGT_DRAW_MAX_SIZE_PX, AGT_DRAW_MAX_SIZE_PX, INT_MAX)) return AGT_DRAW_ERR_ARG;
    if (P < 0 || P > AGT_DRAW_MAX_PRIMS || (long long)B * (long long)P > AGT_DRAW_MAX_TOTAL) return AGT_DRAW_ERR_ARG;
    if (P > 0 && !d_prims) return AGT_DRAW_ERR_ARG;
    if (flags & ~(unsigned)AGT_DRAW_CLEAR) return AGT_DRAW_ERR_ARG;
    if (P == 0 && !(flags & AGT_DRAW_CLEAR)) return AGT_DRAW_OK;

    RasterCall C;
    C.F = agt_side::MutableFrames{ d_frames, pitch, frame_stride, width, height, B };
    C.channels = channels; C.P = P;
    C.prims = d_prims; C.flags = flags;
    const dim3 tiles(div_up(width, TILE_W), div_up(height, TILE_H), 1);
    for (int b0 = 0; b0 < B; b0 += MAX_BATCH_Z) {
        const int nb = B - b0 < MAX_BATCH_Z ? B - b0 : MAX_BATCH_Z;
        hipLaunchKernelGGL(draw_raster_kernel, dim3(tiles.x, tiles.y, nb), dim3(THREADS), 0, (hipStream_t)stream, C, b0);
        if (hipGetLastError() != hipSuccess) return AGT_DRAW_ERR_HIP;
    }
    return AGT_DRAW_OK;
}

int agt_draw_pose_lists(void* stream, const void* d_points, int dtype, int n, int B, const double* d_gate, size_t gate_stride,
                        int width, int height, int corners_per_tag, int radius, int thickness, uint32_t dot_color, uint32_t line_color,
                        agt_draw_prim* d_dots, agt_draw_prim* d_outline)
{
    if (!d_points || !d_dots || !d_outline) return AGT_DRAW_ERR_ARG;
    if (dtype != AGT_DRAW_F32 && dtype != AGT_DRAW_F64) return AGT_DRAW_ERR_ARG;
    if (corners_per_tag != 4 || n < 4 || n > AGT_DRAW_MAX_POINTS || n % 4 != 0) return AGT_DRAW_ERR_ARG;
    if (B < 1 || (long long)B * (long long)n > AGT_DRAW_MAX_TOTAL) return AGT_DRAW_ERR_ARG;
    if (width < 1 || width > AGT_DRAW_MAX_SIZE_PX || height < 1 || height > AGT_DRAW_MAX_SIZE_PX) return AGT_DRAW_ERR_ARG;
    if (radius < 0 || radius > AGT_DRAW_MAX_SIZE || thickness < 0 || thickness > AGT_DRAW_MAX_SIZE) return AGT_DRAW_ERR_ARG;
    if (d_gate && gate_stride < 1) return AGT_DRAW_ERR_ARG;
    if ((dot_color >> 24) || (line_color >> 24)) return AGT_DRAW_ERR_ARG;

    ListCall C;
    C.points = d_points; C.f64 = dtype == AGT_DRAW_F64; C.n = n; C.total = B * n;
    C.gate = d_gate; C.gate_stride = gate_stride;
    C.w = width; C.h = height; C.radius = radius; C.thickness = thickness;
    C.dot_color = dot_color; C.line_color = line_color;
    C.dots = d_dots; C.outline = d_outline;
    hipLaunchKernelGGL(draw_pose_lists_kernel, dim3(div_up(C.total, 256)), dim3(256), 0, (hipStream_t)stream, C);
    if (hipGetLastError() != hipSuccess) return AGT_DRAW_ERR_HIP;
    return AGT_DRAW_OK;
}

}  // extern "C"
