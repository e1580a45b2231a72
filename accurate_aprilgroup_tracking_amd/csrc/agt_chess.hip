// libagt_chess.so (include/agt_chess.h): the X-corners of a chessboard -- corner response, candidates, sub-pixel saddle points.
// One translation unit.  The phases are separate launches on the caller's stream, so the order between them is the stream's:
//   ch_clear        the frames' response maxima set to 0
//   ch_response     one workgroup per TILE_W x TILE_H pixels: the tile and a 5-pixel halo staged in LDS once, the ring read from there;
//                   the workgroup's largest response feeds the frame's atomicMax
//   ch_count        one thread per pixel: the candidate test (thresholds, then the suppression window) into a byte mask, candidates
//                   per AGT_SCAN_CHUNK pixels
//   ch_scan         one workgroup per frame: exclusive scan of those counts (so ids follow raster order), the frame's counts, the
//                   table behind the written candidates zeroed
//   ch_emit         the candidates of a chunk into their places of the table
//   ch_refine       one wave per candidate, four to a workgroup: the saddle-point iteration, the window's samples in LDS
// No kernel waits for another workgroup.  Every loop is a `for` with its bound in the header of the loop.
// Every global write is a vector store or an atomic.
// Shared with the other image stages: the frame arguments and their rule (agt_side_frames.h), the handle's buffers (agt_side_buffers.h),
// the ordered compaction behind ch_count / ch_scan / ch_emit, the fixed-order wave sum and the bilinear fetch (agt_side_device.h).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <math.h>
#include <new>

#include "agt_side_buffers.h"
#include "agt_side_device.h"
#include "agt_side_frames.h"
#include "../../include/agt_chess.h"

#pragma clang fp contract(off)

static_assert(AGT_CHESS_OK == agt_side::OK && AGT_CHESS_ERR_ARG == agt_side::ERR_ARG && AGT_CHESS_ERR_ALLOC == agt_side::ERR_ALLOC &&
              AGT_CHESS_ERR_HIP == agt_side::ERR_HIP, "the codes of agt_side_math.h");
static_assert(sizeof(agt_chess_record) == 48 && sizeof(agt_chess_options) == 40, "the layouts of the header");

namespace {

using agt_side::Frames;
using agt_side::div_up;

constexpr int RING = 5;                                                 // the ring's radius = the halo = the border without a response
constexpr int TILE_W = 64, TILE_H = 16, TILE_PX = TILE_W * TILE_H;      // a response workgroup's pixels
constexpr int STAGE_W = TILE_W + 2 * RING, STAGE_H = TILE_H + 2 * RING, STAGE_PITCH = STAGE_W + 2;        // LDS: 26 x 76 bytes
constexpr int RESP_THREADS = 256, PX_PER_THREAD = TILE_PX / RESP_THREADS;
constexpr int REFINE_WAVES = 4, MAX_WIN = 2 * AGT_CHESS_MAX_HALF + 1, MAX_SAMP = MAX_WIN + 2;             // LDS: 4 x 625 doubles
constexpr int REC_WORDS = sizeof(agt_chess_record) / 4;

__device__ constexpr int RING_X[16] = { 5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2, 0, 2, 4, 5 };
__device__ constexpr int RING_Y[16] = { 0, 2, 4, 5, 5, 5, 4, 2, 0, -2, -4, -5, -5, -5, -4, -2 };

// the workspace, laid out for the call's frame size (n = w * h pixels, nchunk scan chunks per frame)
struct Work {
    int32_t* resp;          // [B][n]
    uint8_t* mask;          // [B][n]: 1 = candidate
    int32_t* chunk;         // [B][nchunk]: candidates of the chunk, then their exclusive prefixes
    int32_t* rmax;          // [B]
    int maxc, nchunk;
};

struct Select { int min_response, rel_pct, nms; };
struct Refine { int half, iters; double max_shift, min_det; double w[MAX_WIN]; };

__device__ __forceinline__ int iabs(int v) { return v < 0 ? -v : v; }

// ---- (a) response

__global__ __launch_bounds__(64) void ch_clear(int32_t* rmax, int B)
{
    if ((int)threadIdx.x < B) rmax[threadIdx.x] = 0;
}

__global__ __launch_bounds__(RESP_THREADS) void ch_response(Frames F, int32_t* resp, int32_t* rmax)
{
    __shared__ uint8_t tile[STAGE_H][STAGE_PITCH];
    __shared__ int best_of[RESP_THREADS / 64];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const uint8_t* img = F.p + (size_t)b * F.stride;
    for (int l = tid; l < STAGE_W * STAGE_H; l += RESP_THREADS) {
        const int ly = l / STAGE_W, lx = l - ly * STAGE_W, x = x0 + lx - RING, y = y0 + ly - RING;
        tile[ly][lx] = x >= 0 && x < F.w && y >= 0 && y < F.h ? img[(size_t)y * F.pitch + x] : (uint8_t)0;
    }
    __syncthreads();
    int best = 0;
#pragma unroll
    for (int j = 0; j < PX_PER_THREAD; j++) {
        const int l = tid + RESP_THREADS * j, lx = l & (TILE_W - 1), ly = l / TILE_W, x = x0 + lx, y = y0 + ly;
        if (x >= F.w || y >= F.h) continue;
        int R = 0;
        if (x >= RING && y >= RING && x < F.w - RING && y < F.h - RING) {
            const int cx = lx + RING, cy = ly + RING;
            int I[16];
#pragma unroll
            for (int k = 0; k < 16; k++) I[k] = tile[cy + RING_Y[k]][cx + RING_X[k]];
            int SR = 0, DR = 0, S = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) SR += iabs(I[k] + I[k + 8] - I[k + 4] - I[k + 12]);
#pragma unroll
            for (int k = 0; k < 8; k++) DR += iabs(I[k] - I[k + 8]);
#pragma unroll
            for (int k = 0; k < 16; k++) S += I[k];
            const int L = tile[cy][cx] + tile[cy][cx - 1] + tile[cy][cx + 1] + tile[cy - 1][cx] + tile[cy + 1][cx];
            R = 5 * (SR - DR) - iabs(5 * S - 16 * L);
        }
        resp[(size_t)b * F.w * F.h + (size_t)y * F.w + x] = R;
        best = R > best ? R : best;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(best, m, 64); best = o > best ? o : best; }
    if ((tid & 63) == 0) best_of[tid >> 6] = best;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int v = 1; v < RESP_THREADS / 64; v++) best = best_of[v] > best ? best_of[v] : best;
        if (best > 0) atomicMax(rmax + b, best);
    }
}

// ---- (b) candidates

__device__ __forceinline__ bool is_candidate(const int32_t* R, int i, int w, int h, int rmax, Select S)
{
    const int r = R[i];
    if (r < S.min_response || 100ll * r < (long long)S.rel_pct * rmax) return false;
    const int y = i / w, x = i - y * w;
    const int ya = y - S.nms > 0 ? y - S.nms : 0, yb = y + S.nms < h - 1 ? y + S.nms : h - 1;
    const int xa = x - S.nms > 0 ? x - S.nms : 0, xb = x + S.nms < w - 1 ? x + S.nms : w - 1;
    bool keep = true;
    for (int yy = ya; yy <= yb; yy++) {                 // at most (2 AGT_CHESS_MAX_NMS + 1)^2 reads
        for (int xx = xa; xx <= xb; xx++) {
            const int j = yy * w + xx, o = R[j];
            keep = keep && (j < i ? o < r : o <= r);
        }
    }
    return keep;
}

__global__ __launch_bounds__(AGT_SCAN_THREADS) void ch_count(Work K, int w, int h, Select S)
{
    __shared__ int part[AGT_SCAN_WAVES];
    const int b = blockIdx.y, n = w * h;
    const int32_t* R = K.resp + (size_t)b * n;
    const int rmax = K.rmax[b];
    int found = 0;
#pragma unroll
    for (int it = 0; it < AGT_SCAN_ITERS; it++) {
        const int i = blockIdx.x * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x;
        const bool c = i < n && is_candidate(R, i, w, h, rmax, S);
        if (i < n) K.mask[(size_t)b * n + i] = c ? 1 : 0;
        found += __popcll(__ballot(c));
    }
    const int total = agt_chunk_total(found, part);
    if (threadIdx.x == 0) K.chunk[(size_t)b * K.nchunk + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void ch_scan(Work K, int32_t* cands, int32_t* counts)
{
    __shared__ int part[4];
    const int b = blockIdx.x;
    int32_t* chunk = K.chunk + (size_t)b * K.nchunk;
    int run = 0;
    for (int base = 0; base < K.nchunk; base += 256) {
        const int i = base + threadIdx.x;
        const int c = i < K.nchunk ? chunk[i] : 0;
        int total;
        const int ex = agt_block_exclusive_sum(c, part, total);
        if (i < K.nchunk) chunk[i] = run + ex;
        run += total;
    }
    const int written = run < K.maxc ? run : K.maxc;
    int32_t* out = cands + (size_t)b * K.maxc * 3;
    for (int at = written * 3 + threadIdx.x; at < K.maxc * 3; at += 256) out[at] = 0;
    if (threadIdx.x == 0) {
        counts[4 * b] = run;
        counts[4 * b + 1] = written;
        counts[4 * b + 2] = K.rmax[b];
        counts[4 * b + 3] = run > K.maxc ? AGT_CHESS_FLAG_CANDIDATES : 0;
    }
}

__global__ __launch_bounds__(AGT_SCAN_THREADS) void ch_emit(Work K, int w, int h, int32_t* cands)
{
    __shared__ int seg[AGT_SCAN_SEGS];
    const int b = blockIdx.y, n = w * h;
    const uint8_t* mask = K.mask + (size_t)b * n;
    int kept[AGT_SCAN_ITERS], below[AGT_SCAN_ITERS];
#pragma unroll
    for (int it = 0; it < AGT_SCAN_ITERS; it++) {
        const int i = blockIdx.x * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x;
        kept[it] = i < n && mask[i] != 0;
        below[it] = agt_chunk_below(kept[it], it, seg);
    }
    __syncthreads();
    const int first = K.chunk[(size_t)b * K.nchunk + blockIdx.x];
#pragma unroll
    for (int it = 0; it < AGT_SCAN_ITERS; it++) {
        if (!kept[it]) continue;
        const int i = blockIdx.x * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x;
        const int id = agt_chunk_rank(first, below[it], it, seg);
        if (id < K.maxc) {
            int32_t* e = cands + ((size_t)b * K.maxc + id) * 3;
            const int y = i / w;
            e[0] = i - y * w; e[1] = y; e[2] = K.resp[(size_t)b * n + i];
        }
    }
}

// ---- (c) the saddle point: one wave per candidate

__global__ __launch_bounds__(64 * REFINE_WAVES) void ch_refine(Frames F, Refine A, const int32_t* cands, const int32_t* counts,
                                                              uint32_t* records, int maxc)
{
    __shared__ double samp[REFINE_WAVES][MAX_SAMP * MAX_SAMP];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, b = blockIdx.y, slot = blockIdx.x * REFINE_WAVES + wave;
    int have = counts[4 * b + 1];
    have = have < 0 ? 0 : have > maxc ? maxc : have;
    const bool mine = slot < maxc, live = slot < have;
    const uint8_t* img = F.p + (size_t)b * F.stride;
    const int n = 2 * A.half + 1, ns = n + 2;
    double sx = 0.0, sy = 0.0;
    if (live) { const int32_t* e = cands + ((size_t)b * maxc + slot) * 3; sx = (double)e[0]; sy = (double)e[1]; }
    double qx = sx, qy = sy, det = 0.0, shift = 0.0;
    int verdict = AGT_CHESS_VERDICT_OK;
    bool running = live;
    // every wave of the workgroup passes both barriers of every iteration, whether it still runs or not
    for (int it = 0; it < A.iters; it++) {
        const double fx = floor(qx), fy = floor(qy);
        if (running && !(fx - (A.half + 1) >= 0.0 && fy - (A.half + 1) >= 0.0 && fx + (A.half + 2) <= (double)(F.w - 1) &&
                         fy + (A.half + 2) <= (double)(F.h - 1))) {
            verdict = AGT_CHESS_VERDICT_BORDER; running = false;
        }
        if (running) {
            const int X = (int)fx, Y = (int)fy;
            const double a = qx - fx, bb = qy - fy;
            for (int t = lane; t < ns * ns; t += 64) {
                const int r = t / ns, c = t - r * ns;
                samp[wave][t] = agt_bilinear_u8(img, F.pitch, X + c - A.half - 1, Y + r - A.half - 1, a, bb);
            }
        }
        __syncthreads();
        if (running) {
            double Sa = 0.0, Sb = 0.0, Sc = 0.0, S1 = 0.0, S2 = 0.0;
            const double* s = samp[wave];
            for (int t = lane; t < n * n; t += 64) {
                const int i = t / n, j = t - i * n;
                const double gx = 0.5 * (s[(i + 1) * ns + j + 2] - s[(i + 1) * ns + j]);
                const double gy = 0.5 * (s[(i + 2) * ns + j + 1] - s[i * ns + j + 1]);
                const double m = A.w[i] * A.w[j], px = (double)(j - A.half), py = (double)(i - A.half);
                const double gxx = gx * gx * m, gxy = gx * gy * m, gyy = gy * gy * m;
                Sa = Sa + gxx; Sb = Sb + gxy; Sc = Sc + gyy;
                S1 = S1 + (gxx * px + gxy * py);
                S2 = S2 + (gxy * px + gyy * py);
            }
            Sa = agt_wave_sum_fixed(Sa); Sb = agt_wave_sum_fixed(Sb); Sc = agt_wave_sum_fixed(Sc); S1 = agt_wave_sum_fixed(S1); S2 = agt_wave_sum_fixed(S2);
            det = Sa * Sc - Sb * Sb;
            if (!(det > A.min_det) || !agt_finite(det)) {
                verdict = AGT_CHESS_VERDICT_FLAT; running = false;
            } else {
                qx = qx + (Sc * S1 - Sb * S2) / det;
                qy = qy + (Sa * S2 - Sb * S1) / det;
                const double dx = qx - sx, dy = qy - sy;
                shift = sqrt(dx * dx + dy * dy);
                if (!(shift <= A.max_shift)) { verdict = AGT_CHESS_VERDICT_SHIFT; running = false; }
            }
        }
        __syncthreads();
    }
    if (!mine || lane != 0) return;
    uint32_t* out = records + ((size_t)b * maxc + slot) * REC_WORDS;
    if (!live) {
#pragma unroll
        for (int k = 0; k < REC_WORDS; k++) out[k] = 0u;
        return;
    }
    if (verdict != AGT_CHESS_VERDICT_OK) { qx = sx; qy = sy; }
    const double d[4] = { qx, qy, det, shift };
#pragma unroll
    for (int k = 0; k < 4; k++) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(d[k]);
        out[2 * k] = (uint32_t)u; out[2 * k + 1] = (uint32_t)(u >> 32);
    }
    out[8] = __float_as_uint((float)qx);
    out[9] = __float_as_uint((float)qy);
    out[10] = (uint32_t)verdict;
    out[11] = 0u;
}

}  // namespace

struct agt_chess {
    AgtSideBuffers buf;
    int width, height, max_batch, maxc;
    Work K;
};

namespace {

// the frame rule against the handle's limits
bool frames_ok(const agt_chess* q, const Frames& F) { return q && agt_side::frames_ok(F.p, F.pitch, F.stride, F.w, F.h, 1, F.B, AGT_CHESS_MIN_SIZE, q->width, q->height, q->max_batch); }

// the defaults with `options` over them; false when a value is outside the header's ranges
bool options_ok(const agt_chess_options* options, agt_chess_options& o)
{
    o.min_response = 200; o.rel_pct = 10; o.nms = 3; o.half = 5; o.iters = 10; o.reserved0 = 0; o.max_shift = 3.0; o.min_det = 1.0;
    if (options) o = *options;
    if (o.min_response < 1 || o.rel_pct < 0 || o.rel_pct > 100 || o.nms < 1 || o.nms > AGT_CHESS_MAX_NMS) return false;
    if (o.half < 1 || o.half > AGT_CHESS_MAX_HALF || o.iters < 1 || o.iters > AGT_CHESS_MAX_ITERS || o.reserved0 != 0) return false;
    if (!(o.max_shift > 0.0 && o.max_shift <= 64.0) || !(o.min_det >= 0.0 && o.min_det <= 1.7976931348623157e308)) return false;
    return true;
}

int enqueue_response(agt_chess* q, hipStream_t s, const Frames& F, int32_t* resp)
{
    hipLaunchKernelGGL(ch_clear, dim3(1), dim3(64), 0, s, q->K.rmax, F.B);
    hipLaunchKernelGGL(ch_response, dim3(div_up(F.w, TILE_W), div_up(F.h, TILE_H), F.B), dim3(RESP_THREADS), 0, s, F, resp, q->K.rmax);
    if (hipGetLastError() != hipSuccess) return AGT_CHESS_ERR_HIP;
    return AGT_CHESS_OK;
}

int enqueue_candidates(agt_chess* q, hipStream_t s, const Frames& F, const agt_chess_options& o, int32_t* cands, int32_t* counts)
{
    RC(enqueue_response(q, s, F, q->K.resp));
    Work K = q->K;
    K.nchunk = div_up((long long)F.w * F.h, AGT_SCAN_CHUNK);
    Select S; S.min_response = o.min_response; S.rel_pct = o.rel_pct; S.nms = o.nms;
    hipLaunchKernelGGL(ch_count, dim3(K.nchunk, F.B), dim3(AGT_SCAN_THREADS), 0, s, K, F.w, F.h, S);
    hipLaunchKernelGGL(ch_scan, dim3(F.B), dim3(256), 0, s, K, cands, counts);
    hipLaunchKernelGGL(ch_emit, dim3(K.nchunk, F.B), dim3(AGT_SCAN_THREADS), 0, s, K, F.w, F.h, cands);
    if (hipGetLastError() != hipSuccess) return AGT_CHESS_ERR_HIP;
    return AGT_CHESS_OK;
}

int enqueue_refine(agt_chess* q, hipStream_t s, const Frames& F, const agt_chess_options& o, const int32_t* cands, const int32_t* counts,
                   agt_chess_record* records)
{
    Refine A;
    A.half = o.half; A.iters = o.iters; A.max_shift = o.max_shift; A.min_det = o.min_det;
    for (int i = 0; i < MAX_WIN; i++) {
        const double x = (double)(i - o.half) / (double)o.half;
        A.w[i] = i < 2 * o.half + 1 ? exp(-(x * x)) : 0.0;
    }
    hipLaunchKernelGGL(ch_refine, dim3(div_up(q->maxc, REFINE_WAVES), F.B), dim3(64 * REFINE_WAVES), 0, s, F, A, cands, counts,
                       reinterpret_cast<uint32_t*>(records), q->maxc);
    if (hipGetLastError() != hipSuccess) return AGT_CHESS_ERR_HIP;
    return AGT_CHESS_OK;
}

}  // namespace

extern "C" {

int agt_chess_version(void) { return AGT_CHESS_VERSION; }

int agt_chess_create(int width, int height, int max_batch, int max_candidates, agt_chess** handle_out)
{
    if (!handle_out) return AGT_CHESS_ERR_ARG;
    *handle_out = nullptr;
    if (width < AGT_CHESS_MIN_SIZE || width > AGT_CHESS_MAX_SIZE || height < AGT_CHESS_MIN_SIZE || height > AGT_CHESS_MAX_SIZE) return AGT_CHESS_ERR_ARG;
    if (max_batch < 1 || max_batch > AGT_CHESS_MAX_BATCH) return AGT_CHESS_ERR_ARG;
    if (max_candidates < 1 || max_candidates > AGT_CHESS_MAX_CANDIDATES) return AGT_CHESS_ERR_ARG;
    agt_chess* q = new (std::nothrow) agt_chess();
    if (!q) return AGT_CHESS_ERR_ALLOC;
    q->width = width; q->height = height; q->max_batch = max_batch; q->maxc = max_candidates;
    const size_t B = (size_t)max_batch, n = (size_t)width * height, nc = (size_t)div_up((long long)n, AGT_SCAN_CHUNK);
    Work& K = q->K;
    K.maxc = max_candidates; K.nchunk = 0;
    AgtSideBuffers& m = q->buf;
    if (m.alloc_n(&K.resp, B * n) || m.alloc_n(&K.mask, B * n) || m.alloc_n(&K.chunk, B * nc) || m.alloc_n(&K.rmax, B)) {
        agt_side_destroy(q);
        return AGT_CHESS_ERR_ALLOC;
    }
    *handle_out = q;
    return AGT_CHESS_OK;
}

int agt_chess_destroy(agt_chess* handle) { return agt_side_destroy(handle); }

int agt_chess_response(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                       int B, int32_t* d_response)
{
    const Frames F = { d_frames, pitch, frame_stride, width, height, B };
    if (!frames_ok(handle, F) || !d_response) return AGT_CHESS_ERR_ARG;
    return enqueue_response(handle, (hipStream_t)stream, F, d_response);
}

int agt_chess_candidates(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                         int B, const agt_chess_options* options, int32_t* d_candidates, int32_t* d_counts)
{
    const Frames F = { d_frames, pitch, frame_stride, width, height, B };
    agt_chess_options o;
    if (!frames_ok(handle, F) || !d_candidates || !d_counts || !options_ok(options, o)) return AGT_CHESS_ERR_ARG;
    return enqueue_candidates(handle, (hipStream_t)stream, F, o, d_candidates, d_counts);
}

int agt_chess_refine(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                     int B, const agt_chess_options* options, const int32_t* d_candidates, const int32_t* d_counts,
                     agt_chess_record* d_records)
{
    const Frames F = { d_frames, pitch, frame_stride, width, height, B };
    agt_chess_options o;
    if (!frames_ok(handle, F) || !d_candidates || !d_counts || !d_records || !options_ok(options, o)) return AGT_CHESS_ERR_ARG;
    return enqueue_refine(handle, (hipStream_t)stream, F, o, d_candidates, d_counts, d_records);
}

int agt_chess_corners(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                      int B, const agt_chess_options* options, int32_t* d_candidates, int32_t* d_counts, agt_chess_record* d_records)
{
    const Frames F = { d_frames, pitch, frame_stride, width, height, B };
    agt_chess_options o;
    if (!frames_ok(handle, F) || !d_candidates || !d_counts || !d_records || !options_ok(options, o)) return AGT_CHESS_ERR_ARG;
    RC(enqueue_candidates(handle, (hipStream_t)stream, F, o, d_candidates, d_counts));
    return enqueue_refine(handle, (hipStream_t)stream, F, o, d_candidates, d_counts, d_records);
}

}  // extern "C"
