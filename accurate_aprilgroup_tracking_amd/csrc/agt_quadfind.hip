// libagt_quadfind.so (include/agt_quadfind.h): the first stage of a tag detector -- threshold, component labelling, quad extraction.
// One translation unit.  The phases are separate launches on the caller's stream, so the order between them is the stream's:
//   qf_tile_minmax    one thread per 4 x 4 tile: its smallest and largest pixel
//   qf_tile_neigh     one thread per tile: smallest / largest over the 3 x 3 tile neighbourhood
//   qf_label_tiles    one workgroup per TILE_W x TILE_H pixels: threshold, union-find in LDS, labels as global indices, the tile's areas
//   qf_merge_borders  one thread per pixel on a workgroup-tile border: union with the pixel across the border (atomicMin, global)
//   qf_flatten_area   one thread per pixel: label = root; a tile's root adds the tile's share of the area to the component's root
//   qf_root_count     roots and roots inside the area limits per AGT_SCAN_CHUNK pixels
//   qf_root_scan      one workgroup per frame: exclusive scan of those counts (ids follow label order), counts[0..1]
//   qf_root_assign    the compact id of every root inside the area limits; its row of the component table set to the identities
//   qf_support        one thread per pixel: the pixels of table components that can be extreme in a direction feed its atomicMax,
//                     reduced within the wave first for up to SUPPORT_ROUNDS components per wave
//   qf_quads          one thread per table component: the 16 support points (in LDS) reduced to four vertices, the bounding box
//                     read off the four axis directions, the filters
//   qf_emit           one workgroup per frame: ordered compaction of the candidates into the outputs, the rest zeroed, counts[2..3]
// No kernel waits for another workgroup.  Every loop is a `for` with its bound in the header of the loop.  The union-find keeps
// parent[i] <= i: find walks strictly decreasing indices, a merge is atomicMin on the larger root, so it ends without a lock; a stale
// read only costs a step, never a wrong answer (the atomicMin's return value decides).
// Every global write is a vector store or an atomic.
// Shared with the other image stages: the frame arguments and their rule (agt_side_frames.h), the handle's buffers (agt_side_buffers.h),
// the ordered compaction behind qf_root_count / _scan / _assign and qf_emit (agt_side_device.h; no floating point here: no mode re-stated).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <limits.h>
#include <new>

#include "agt_side_buffers.h"
#include "agt_side_device.h"
#include "agt_side_frames.h"
#include "../../include/agt_quadfind.h"

static_assert(AGT_QUADFIND_OK == agt_side::OK && AGT_QUADFIND_ERR_ARG == agt_side::ERR_ARG && AGT_QUADFIND_ERR_ALLOC == agt_side::ERR_ALLOC &&
              AGT_QUADFIND_ERR_HIP == agt_side::ERR_HIP, "the codes of agt_side_math.h");
static_assert(sizeof(agt_quadfind_record) == 32 && sizeof(agt_quadfind_options) == 16, "the layouts of the header");

namespace {

using agt_side::Frames;
using agt_side::div_up;

constexpr int TILE_W = 64, TILE_H = 16, TILE_PX = TILE_W * TILE_H;     // a labelling workgroup's pixels (LDS: 8 KiB)
constexpr int SUPPORT_ROUNDS = 4;
constexpr int LABEL_THREADS = 256, PX_PER_THREAD = TILE_PX / LABEL_THREADS;
constexpr int PROJ_BIAS = 1 << 26;      // |x dx + y dy| <= 2 * 8192 * 1024 = 2^24
constexpr int MIN_EDGE_SQ = 64;

__device__ constexpr int DIR_X[16] = { 1024, 946, 724, 392, 0, -392, -724, -946, -1024, -946, -724, -392, 0, 392, 724, 946 };
__device__ constexpr int DIR_Y[16] = { 0, 392, 724, 946, 1024, 946, 724, 392, 0, -392, -724, -946, -1024, -946, -724, -392 };

// the workspace, laid out for the call's frame size (n = w * h pixels, nt = th * tw tiles, nchunk scan chunks per frame)
struct Work {
    uint8_t *mn, *mx, *MN, *MX;         // [B][nt]
    int32_t *label, *area, *cid;        // [B][n]; cid is written and read at roots only
    int2* chunk;                        // [B][nchunk]: (roots, roots inside the area limits), then exclusive prefixes of the second
    int32_t *c_root, *c_area;           // [B][maxc]
    unsigned long long* c_sup;          // [B][maxc][16]
    int32_t* c_valid;                   // [B][maxc]
    float* c_quad;                      // [B][maxc][8]
    agt_quadfind_record* c_rec;         // [B][maxc]
    int maxc, maxq, nchunk;
};

// ---- union-find on parent[i] <= i, -1 = not dark

template <typename P>
__device__ __forceinline__ int uf_load(P* parent, int i)
{
    return __hip_atomic_load(parent + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x among n elements: at most n steps, each to a strictly smaller index
__device__ __forceinline__ int uf_find(int* parent, int x, int n)
{
    for (int it = 0; it < n; it++) {
        const int p = uf_load(parent, x);
        if (p >= x) break;
        x = p;
    }
    return x;
}

// Joins the sets of a and b.  Each round either ends or lowers max(a, b): at most n rounds.
__device__ __forceinline__ void uf_union(int* parent, int a, int b, int n)
{
    for (int it = 0; it < n; it++) {
        a = uf_find(parent, a, n);
        b = uf_find(parent, b, n);
        if (a == b) return;
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);
        if (old == a) return;           // a was a root and now hangs under b
        a = old;                        // somebody moved a first: what it hung under (old < a) still has to meet b
    }
}

// ---- (a) tile minima and maxima

__global__ __launch_bounds__(256) void qf_tile_minmax(Frames F, Work K, int th, int tw)
{
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= th * tw) return;
    const int ty = t / tw, tx = t - ty * tw;
    const uint8_t* p = F.p + (size_t)b * F.stride + (size_t)(4 * ty) * F.pitch + (size_t)(4 * tx);
    int lo = 255, hi = 0;
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const int v = p[(size_t)r * F.pitch + c];
            lo = v < lo ? v : lo; hi = v > hi ? v : hi;
        }
    }
    K.mn[(size_t)b * th * tw + t] = (uint8_t)lo;
    K.mx[(size_t)b * th * tw + t] = (uint8_t)hi;
}

__global__ __launch_bounds__(256) void qf_tile_neigh(Work K, int th, int tw)
{
    const int t = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y;
    if (t >= th * tw) return;
    const int ty = t / tw, tx = t - ty * tw;
    const uint8_t *mn = K.mn + (size_t)b * th * tw, *mx = K.mx + (size_t)b * th * tw;
    int lo = 255, hi = 0;
#pragma unroll
    for (int dy = -1; dy <= 1; dy++) {
#pragma unroll
        for (int dx = -1; dx <= 1; dx++) {
            const int y = ty + dy, x = tx + dx;
            if (y >= 0 && y < th && x >= 0 && x < tw) {
                const int a = mn[y * tw + x], c = mx[y * tw + x];
                lo = a < lo ? a : lo; hi = c > hi ? c : hi;
            }
        }
    }
    K.MN[(size_t)b * th * tw + t] = (uint8_t)lo;
    K.MX[(size_t)b * th * tw + t] = (uint8_t)hi;
}

// ---- (b) threshold and labelling of one TILE_W x TILE_H tile in LDS

__global__ __launch_bounds__(LABEL_THREADS) void qf_label_tiles(Frames F, Work K, int32_t* label, int th, int tw, int min_contrast)
{
    __shared__ int par[TILE_PX], cnt[TILE_PX];
    const int tid = threadIdx.x, b = blockIdx.z;
    const int x0 = blockIdx.x * TILE_W, y0 = blockIdx.y * TILE_H;
    const uint8_t* img = F.p + (size_t)b * F.stride;
    const uint8_t *MN = K.MN + (size_t)b * th * tw, *MX = K.MX + (size_t)b * th * tw;
    bool dark[PX_PER_THREAD];
#pragma unroll
    for (int j = 0; j < PX_PER_THREAD; j++) {
        const int l = tid + LABEL_THREADS * j, x = x0 + (l & (TILE_W - 1)), y = y0 + l / TILE_W;
        dark[j] = false;
        if (x < F.w && y < F.h) {
            const int v = img[(size_t)y * F.pitch + x];
            const int ty = (y >> 2) < th - 1 ? (y >> 2) : th - 1, tx = (x >> 2) < tw - 1 ? (x >> 2) : tw - 1;
            const int lo = MN[ty * tw + tx], hi = MX[ty * tw + tx];
            dark[j] = hi - lo >= min_contrast && 2 * v < lo + hi;
        }
        par[l] = dark[j] ? l : -1;
        cnt[l] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PX_PER_THREAD; j++) {
        const int l = tid + LABEL_THREADS * j;
        if (dark[j]) {
            if ((l & (TILE_W - 1)) != 0 && uf_load(par, l - 1) >= 0) uf_union(par, l, l - 1, TILE_PX);
            if (l >= TILE_W && uf_load(par, l - TILE_W) >= 0) uf_union(par, l, l - TILE_W, TILE_PX);
        }
    }
    __syncthreads();
    int root[PX_PER_THREAD];
#pragma unroll
    for (int j = 0; j < PX_PER_THREAD; j++) {
        root[j] = dark[j] ? uf_find(par, tid + LABEL_THREADS * j, TILE_PX) : -1;
        if (dark[j]) atomicAdd(cnt + root[j], 1);       // the tile's share of the area, kept at the tile's root
    }
    __syncthreads();
#pragma unroll
    for (int j = 0; j < PX_PER_THREAD; j++) {
        const int l = tid + LABEL_THREADS * j, x = x0 + (l & (TILE_W - 1)), y = y0 + l / TILE_W;
        if (x < F.w && y < F.h) {
            const size_t at = (size_t)b * F.w * F.h + (size_t)y * F.w + x;
            label[at] = dark[j] ? (y0 + root[j] / TILE_W) * F.w + x0 + (root[j] & (TILE_W - 1)) : -1;
            K.area[at] = cnt[l];            // (0 anywhere but at a root of this tile)
        }
    }
}

// ---- (c) merges across the borders of those tiles

__global__ __launch_bounds__(256) void qf_merge_borders(int32_t* label, int w, int h)
{
    const int ncol = (w - 1) / TILE_W, nrow = (h - 1) / TILE_H;        // vertical borders at x = TILE_W i, horizontal ones at y = TILE_H j
    const int nv = ncol * h, nh = nrow * w;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= nv + nh) return;
    int* L = label + (size_t)blockIdx.y * w * h;
    int x, y, other;
    if (t < nv) { x = TILE_W * (t / h + 1); y = t % h; other = y * w + x - 1; }
    else { const int u = t - nv; y = TILE_H * (u / w + 1); x = u % w; other = (y - 1) * w + x; }
    const int me = y * w + x;
    if (uf_load(L, me) >= 0 && uf_load(L, other) >= 0) uf_union(L, me, other, w * h);
}

// ---- (d) flatten, areas

__global__ __launch_bounds__(256) void qf_flatten_area(int32_t* label, Work K, int n)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int* L = label + (size_t)blockIdx.y * n;
    if (L[i] < 0) return;
    const int r = uf_find(L, i, n);
    L[i] = r;                       // (a walk that passes here meets the root sooner; roots do not change in this kernel)
    // a tile's root that is not the component's hands the tile's share on: one atomic per tile and component, and nobody adds to
    // area[i] here, since additions go to final roots only
    int32_t* area = K.area + (size_t)blockIdx.y * n;
    const int share = area[i];
    if (share > 0 && r != i) atomicAdd(area + r, share);
}

// a root inside the area limits?  (.x: root, .y: kept)
__device__ __forceinline__ int2 root_kind(const int32_t* L, const int32_t* area, int i, int n, int min_area, int max_area)
{
    int2 k = make_int2(0, 0);
    if (i < n && L[i] == i) {
        const int a = area[i];
        k.x = 1;
        k.y = a >= min_area && a <= max_area;
    }
    return k;
}

__global__ __launch_bounds__(AGT_SCAN_THREADS) void qf_root_count(Work K, int n, int min_area, int max_area)
{
    __shared__ int2 part[AGT_SCAN_WAVES];
    const int b = blockIdx.y;
    const int32_t *L = K.label + (size_t)b * n, *area = K.area + (size_t)b * n;
    int roots = 0, kept = 0;
#pragma unroll
    for (int it = 0; it < AGT_SCAN_ITERS; it++) {
        const int2 k = root_kind(L, area, blockIdx.x * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x, n, min_area, max_area);
        roots += __popcll(__ballot(k.x));
        kept += __popcll(__ballot(k.y));
    }
    const int2 total = agt_chunk_total(make_int2(roots, kept), part);
    if (threadIdx.x == 0) K.chunk[(size_t)b * K.nchunk + blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void qf_root_scan(Work K, int32_t* counts)
{
    __shared__ int part[4], rpart[4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int2* chunk = K.chunk + (size_t)b * K.nchunk;
    int run = 0, roots = 0;
    for (int base = 0; base < K.nchunk; base += 256) {
        const int i = base + threadIdx.x;
        const int2 c = i < K.nchunk ? chunk[i] : make_int2(0, 0);
        int total;
        const int ex = agt_block_exclusive_sum(c.y, part, total);
        if (i < K.nchunk) chunk[i].y = run + ex;
        run += total;
        int r = c.x;
#pragma unroll
        for (int m = 32; m >= 1; m >>= 1) r += __shfl_xor(r, m, 64);
        if (lane == 0) rpart[wave] = r;
        __syncthreads();
        roots += rpart[0] + rpart[1] + rpart[2] + rpart[3];
    }
    if (threadIdx.x == 0) { counts[4 * b] = roots; counts[4 * b + 1] = run; }
}

__global__ __launch_bounds__(AGT_SCAN_THREADS) void qf_root_assign(Work K, int n, int min_area, int max_area)
{
    __shared__ int seg[AGT_SCAN_SEGS];
    const int b = blockIdx.y;
    const int32_t *L = K.label + (size_t)b * n, *area = K.area + (size_t)b * n;
    int kept[AGT_SCAN_ITERS], below[AGT_SCAN_ITERS];
#pragma unroll
    for (int it = 0; it < AGT_SCAN_ITERS; it++) {
        kept[it] = root_kind(L, area, blockIdx.x * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x, n, min_area, max_area).y;
        below[it] = agt_chunk_below(kept[it], it, seg);
    }
    __syncthreads();
    const int first = K.chunk[(size_t)b * K.nchunk + blockIdx.x].y;
#pragma unroll
    for (int it = 0; it < AGT_SCAN_ITERS; it++) {
        if (!kept[it]) continue;
        const int i = blockIdx.x * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x;
        const int id = agt_chunk_rank(first, below[it], it, seg);
        const bool in = id < K.maxc;
        K.cid[(size_t)b * n + i] = in ? id : -1;
        if (in) {
            const size_t c = (size_t)b * K.maxc + id;
            K.c_root[c] = i;
            K.c_area[c] = area[i];
#pragma unroll
            for (int k = 0; k < 16; k++) K.c_sup[16 * c + k] = 0ull;
        }
    }
    // a root outside the area limits: no id
#pragma unroll
    for (int it = 0; it < AGT_SCAN_ITERS; it++) {
        const int i = blockIdx.x * AGT_SCAN_CHUNK + it * AGT_SCAN_THREADS + threadIdx.x;
        if (!kept[it] && i < n && L[i] == i) K.cid[(size_t)b * n + i] = -1;
    }
}

// ---- (e) support points and bounding boxes

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const unsigned long long o = __shfl_xor(v, m, 64);
        v = o > v ? o : v;
    }
    return v;
}

__global__ __launch_bounds__(256) void qf_support(Work K, int w, int h)
{
    const int n = w * h, i = blockIdx.x * 256 + threadIdx.x, b = blockIdx.y, lane = threadIdx.x & 63;
    const int32_t* L = K.label + (size_t)b * n;
    int c = -1, x = 0, y = 0;
    bool right = false, left = false, down = false, up = false;         // the dark neighbours
    if (i < n) {
        const int r = L[i];
        if (r >= 0) {
            y = i / w; x = i - y * w;
            right = x < w - 1 && L[i + 1] >= 0; left = x > 0 && L[i - 1] >= 0;
            down = y < h - 1 && L[i + w] >= 0; up = y > 0 && L[i - w] >= 0;
            // a pixel with four dark neighbours is extreme in no direction
            if (!(right && left && down && up)) c = K.cid[(size_t)b * n + r];
        }
    }
    bool pending = c >= 0;
    if (__ballot(pending) == 0ull) return;
    const unsigned int low = 0xFFFFFFFFu - (unsigned int)i;
    // the components of the wave one after the other, each reduced within the wave before its atomics ...
    for (int round = 0; round < SUPPORT_ROUNDS; round++) {
        const unsigned long long m = __ballot(pending);
        if (m == 0ull) return;
        const int lead = __ffsll((long long)m) - 1;
        const int c0 = __shfl(c, lead, 64);
        const bool mine = pending && c == c0;
        unsigned long long* sup = K.c_sup + 16 * ((size_t)b * K.maxc + (size_t)c0);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            // a dark neighbour on the side the direction points to projects further: this pixel is not the support point
            const bool beaten = (DIR_X[k] > 0 && right) || (DIR_X[k] < 0 && left) || (DIR_Y[k] > 0 && down) || (DIR_Y[k] < 0 && up);
            const unsigned int proj = (unsigned int)(x * DIR_X[k] + y * DIR_Y[k] + PROJ_BIAS);
            const unsigned long long key = wave_max_u64(mine && !beaten ? ((unsigned long long)proj << 32) | low : 0ull);
            if (lane == lead && key != 0ull) atomicMax(sup + k, key);
        }
        pending = pending && !mine;
    }
    // ... and what is left in a wave that holds more components than that, each pixel for itself (little contention: many owners)
    if (pending) {
        unsigned long long* sup = K.c_sup + 16 * ((size_t)b * K.maxc + (size_t)c);
#pragma unroll
        for (int k = 0; k < 16; k++) {
            const bool beaten = (DIR_X[k] > 0 && right) || (DIR_X[k] < 0 && left) || (DIR_Y[k] > 0 && down) || (DIR_Y[k] < 0 && up);
            const unsigned int proj = (unsigned int)(x * DIR_X[k] + y * DIR_Y[k] + PROJ_BIAS);
            if (!beaten) atomicMax(sup + k, ((unsigned long long)proj << 32) | low);
        }
    }
}

// ---- (f) quad extraction: one thread per component of the table, its vertex list in LDS (indexed, so not in registers)

__device__ __forceinline__ long long cross3(int ax, int ay, int bx, int by, int cx, int cy)
{
    return (long long)(bx - ax) * (long long)(cy - ay) - (long long)(by - ay) * (long long)(cx - ax);
}

__global__ __launch_bounds__(64) void qf_quads(Work K, const int32_t* counts, int w, int h, int min_fill_pct)
{
    __shared__ int px[16][64], py[16][64];
    const int t = threadIdx.x, b = blockIdx.y, id = blockIdx.x * 64 + t;
    const int have = counts[4 * b + 1] < K.maxc ? counts[4 * b + 1] : K.maxc;
    if (id >= have) return;
    const size_t c = (size_t)b * K.maxc + id;
    int nv = 0;
#pragma unroll
    for (int k = 0; k < 16; k++) {
        const unsigned int at = 0xFFFFFFFFu - (unsigned int)K.c_sup[16 * c + k];
        const int y = (int)(at / (unsigned int)w), x = (int)(at - (unsigned int)y * (unsigned int)w);
        if (nv == 0 || x != px[nv - 1][t] || y != py[nv - 1][t]) { px[nv][t] = x; py[nv][t] = y; nv++; }
    }
    if (nv > 1 && px[nv - 1][t] == px[0][t] && py[nv - 1][t] == py[0][t]) nv--;
    for (int it = 0; it < 12 && nv > 4; it++) {                 // 16 vertices at most: 12 removals at most
        long long best = LLONG_MAX;
        int at = 0;
        for (int i = 0; i < nv; i++) {
            const int p = i == 0 ? nv - 1 : i - 1, q = i == nv - 1 ? 0 : i + 1;
            long long a = cross3(px[p][t], py[p][t], px[i][t], py[i][t], px[q][t], py[q][t]);
            a = a < 0 ? -a : a;
            if (a < best) { best = a; at = i; }
        }
        for (int i = at; i < nv - 1; i++) { px[i][t] = px[i + 1][t]; py[i][t] = py[i + 1][t]; }
        nv--;
    }
    const int area = K.c_area[c];
    // the bounding box is what the four axis directions found: k = 0 / 4 / 8 / 12 maximise x, y, -x, -y
    const unsigned int ex1 = 0xFFFFFFFFu - (unsigned int)K.c_sup[16 * c + 0], ey1 = 0xFFFFFFFFu - (unsigned int)K.c_sup[16 * c + 4];
    const unsigned int ex0 = 0xFFFFFFFFu - (unsigned int)K.c_sup[16 * c + 8], ey0 = 0xFFFFFFFFu - (unsigned int)K.c_sup[16 * c + 12];
    const int x1 = (int)(ex1 % (unsigned int)w), y1 = (int)(ey1 / (unsigned int)w), x0 = (int)(ex0 % (unsigned int)w), y0 = (int)(ey0 / (unsigned int)w);
    bool good = x0 > 0 && y0 > 0 && x1 < w - 1 && y1 < h - 1 && nv == 4;
    int vx[4] = { 0, 0, 0, 0 }, vy[4] = { 0, 0, 0, 0 };
    long long s2 = 0;
    if (good) {
#pragma unroll
        for (int j = 0; j < 4; j++) { vx[j] = px[j][t]; vy[j] = py[j][t]; }
#pragma unroll
        for (int j = 0; j < 4; j++) s2 += (long long)vx[j] * vy[(j + 1) & 3] - (long long)vx[(j + 1) & 3] * vy[j];
        s2 = s2 < 0 ? -s2 : s2;
        good = s2 > 0 && 200ll * area >= (long long)min_fill_pct * s2 && 20ll * area <= 11ll * s2 + 400ll;
        bool pos = true, neg = true;
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int k = (j + 1) & 3, l = (j + 2) & 3;
            const long long cr = (long long)(vx[k] - vx[j]) * (vy[l] - vy[k]) - (long long)(vy[k] - vy[j]) * (vx[l] - vx[k]);
            pos = pos && cr > 0; neg = neg && cr < 0;
            const long long ex = vx[k] - vx[j], ey = vy[k] - vy[j];
            good = good && ex * ex + ey * ey >= MIN_EDGE_SQ;
        }
        good = good && (pos || neg);
    }
    K.c_valid[c] = good ? 1 : 0;
    if (good) {
        const int sx = vx[0] + vx[1] + vx[2] + vx[3], sy = vy[0] + vy[1] + vy[2] + vy[3];
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const int dx = 4 * vx[j] - sx, dy = 4 * vy[j] - sy;
            K.c_quad[8 * c + 2 * j] = (float)vx[j] + (dx > 0 ? 0.5f : dx < 0 ? -0.5f : 0.0f);
            K.c_quad[8 * c + 2 * j + 1] = (float)vy[j] + (dy > 0 ? 0.5f : dy < 0 ? -0.5f : 0.0f);
        }
        agt_quadfind_record r;
        r.label = K.c_root[c]; r.area = area; r.x0 = x0; r.y0 = y0; r.x1 = x1; r.y1 = y1; r.s2 = s2;
        K.c_rec[c] = r;
    }
}

// ---- ordered compaction into the caller's arrays

__global__ __launch_bounds__(256) void qf_emit(Work K, uint32_t* quads, uint32_t* rec, int32_t* counts)
{
    __shared__ int part[4];
    const int b = blockIdx.x;
    const int all = counts[4 * b + 1], have = all < K.maxc ? all : K.maxc;
    // both outputs as 32-bit words (eight per entry): the caller's arrays need no more than 4-byte alignment
    uint32_t *oq = quads + (size_t)b * K.maxq * 8, *orec = rec + (size_t)b * K.maxq * 8;
    const uint32_t* iq = reinterpret_cast<const uint32_t*>(K.c_quad) + (size_t)b * K.maxc * 8;
    const uint32_t* irec = reinterpret_cast<const uint32_t*>(K.c_rec) + (size_t)b * K.maxc * 8;
    int run = 0;
    for (int base = 0; base < have; base += 256) {
        const int id = base + threadIdx.x;
        const int v = id < have ? K.c_valid[(size_t)b * K.maxc + id] : 0;
        int total;
        const int at = run + agt_block_exclusive_sum(v, part, total);
        if (v && at < K.maxq) {
#pragma unroll
            for (int j = 0; j < 8; j++) { oq[8 * (size_t)at + j] = iq[8 * (size_t)id + j]; orec[8 * (size_t)at + j] = irec[8 * (size_t)id + j]; }
        }
        run += total;
    }
    const int written = run < K.maxq ? run : K.maxq;
    for (int at = written * 8 + threadIdx.x; at < K.maxq * 8; at += 256) { oq[at] = 0u; orec[at] = 0u; }
    if (threadIdx.x == 0) {
        counts[4 * b + 2] = run;
        counts[4 * b + 3] = (run > K.maxq ? AGT_QUADFIND_FLAG_QUADS : 0) | (all > K.maxc ? AGT_QUADFIND_FLAG_COMPONENTS : 0);
    }
}

}  // namespace

struct agt_quadfind {
    AgtSideBuffers buf;
    int width, height, max_batch, maxc, maxq;
    Work K;
};

namespace {

// the frame rule against the handle's limits
bool frames_ok(const agt_quadfind* q, const Frames& F) { return q && agt_side::frames_ok(F.p, F.pitch, F.stride, F.w, F.h, 1, F.B, AGT_QUADFIND_MIN_SIZE, q->width, q->height, q->max_batch); }

// steps 1 and 2 of the rule into `label` ([B][h][w])
int enqueue_labels(agt_quadfind* q, hipStream_t s, const Frames& F, int min_contrast, int32_t* label)
{
    const int th = F.h / 4, tw = F.w / 4, n = F.w * F.h;
    hipLaunchKernelGGL(qf_tile_minmax, dim3(div_up(th * tw, 256), F.B), dim3(256), 0, s, F, q->K, th, tw);
    hipLaunchKernelGGL(qf_tile_neigh, dim3(div_up(th * tw, 256), F.B), dim3(256), 0, s, q->K, th, tw);
    hipLaunchKernelGGL(qf_label_tiles, dim3(div_up(F.w, TILE_W), div_up(F.h, TILE_H), F.B), dim3(LABEL_THREADS), 0, s, F, q->K, label, th, tw, min_contrast);
    const int borders = ((F.w - 1) / TILE_W) * F.h + ((F.h - 1) / TILE_H) * F.w;
    if (borders > 0) hipLaunchKernelGGL(qf_merge_borders, dim3(div_up(borders, 256), F.B), dim3(256), 0, s, label, F.w, F.h);
    hipLaunchKernelGGL(qf_flatten_area, dim3(div_up(n, 256), F.B), dim3(256), 0, s, label, q->K, n);
    if (hipGetLastError() != hipSuccess) return AGT_QUADFIND_ERR_HIP;
    return AGT_QUADFIND_OK;
}

}  // namespace

extern "C" {

int agt_quadfind_version(void) { return AGT_QUADFIND_VERSION; }

int agt_quadfind_create(int width, int height, int max_batch, int max_components, int max_quads, agt_quadfind** handle_out)
{
    if (!handle_out) return AGT_QUADFIND_ERR_ARG;
    *handle_out = nullptr;
    if (width < AGT_QUADFIND_MIN_SIZE || width > AGT_QUADFIND_MAX_SIZE || height < AGT_QUADFIND_MIN_SIZE || height > AGT_QUADFIND_MAX_SIZE) return AGT_QUADFIND_ERR_ARG;
    if (max_batch < 1 || max_batch > AGT_QUADFIND_MAX_BATCH) return AGT_QUADFIND_ERR_ARG;
    if (max_components < 1 || max_components > AGT_QUADFIND_MAX_COMPONENTS || max_quads < 1 || max_quads > max_components) return AGT_QUADFIND_ERR_ARG;
    agt_quadfind* q = new (std::nothrow) agt_quadfind();
    if (!q) return AGT_QUADFIND_ERR_ALLOC;
    q->width = width; q->height = height; q->max_batch = max_batch; q->maxc = max_components; q->maxq = max_quads;
    const size_t B = (size_t)max_batch, n = (size_t)width * height, nt = (size_t)(width / 4) * (height / 4), nc = (size_t)div_up((long long)n, AGT_SCAN_CHUNK);
    const size_t mc = (size_t)max_components;
    Work& K = q->K;
    K.maxc = max_components; K.maxq = max_quads; K.nchunk = 0;
    AgtSideBuffers& m = q->buf;
    if (m.alloc_n(&K.mn, B * nt) || m.alloc_n(&K.mx, B * nt) || m.alloc_n(&K.MN, B * nt) || m.alloc_n(&K.MX, B * nt) ||
        m.alloc_n(&K.label, B * n) || m.alloc_n(&K.area, B * n) || m.alloc_n(&K.cid, B * n) ||
        m.alloc_n(&K.chunk, B * nc) ||
        m.alloc_n(&K.c_root, B * mc) || m.alloc_n(&K.c_area, B * mc) || m.alloc_n(&K.c_sup, B * mc * 16) ||
        m.alloc_n(&K.c_valid, B * mc) || m.alloc_n(&K.c_quad, B * mc * 8) || m.alloc_n(&K.c_rec, B * mc)) {
        agt_side_destroy(q);
        return AGT_QUADFIND_ERR_ALLOC;
    }
    *handle_out = q;
    return AGT_QUADFIND_OK;
}

int agt_quadfind_destroy(agt_quadfind* handle) { return agt_side_destroy(handle); }

int agt_quadfind_labels(agt_quadfind* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width,
                        int height, int B, int min_contrast, int32_t* d_labels)
{
    const Frames F = { d_frames, pitch, frame_stride, width, height, B };
    if (!frames_ok(handle, F) || !d_labels) return AGT_QUADFIND_ERR_ARG;
    if (min_contrast < 1 || min_contrast > 255) return AGT_QUADFIND_ERR_ARG;
    return enqueue_labels(handle, (hipStream_t)stream, F, min_contrast, d_labels);
}

int agt_quadfind_detect(agt_quadfind* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width,
                        int height, int B, const agt_quadfind_options* options, float* d_quads, agt_quadfind_record* d_records,
                        int32_t* d_counts)
{
    const Frames F = { d_frames, pitch, frame_stride, width, height, B };
    if (!frames_ok(handle, F) || !d_quads || !d_records || !d_counts) return AGT_QUADFIND_ERR_ARG;
    agt_quadfind_options o;
    o.min_contrast = 40; o.min_area = 24; o.max_area = INT32_MAX; o.min_fill_pct = 5;
    if (options) o = *options;
    if (o.min_contrast < 1 || o.min_contrast > 255 || o.min_area < 1 || o.max_area < o.min_area || o.min_fill_pct < 0 || o.min_fill_pct > 100) return AGT_QUADFIND_ERR_ARG;
    hipStream_t s = (hipStream_t)stream;
    RC(enqueue_labels(handle, s, F, o.min_contrast, handle->K.label));
    Work K = handle->K;
    const int n = width * height;
    K.nchunk = div_up(n, AGT_SCAN_CHUNK);
    hipLaunchKernelGGL(qf_root_count, dim3(K.nchunk, B), dim3(AGT_SCAN_THREADS), 0, s, K, n, o.min_area, o.max_area);
    hipLaunchKernelGGL(qf_root_scan, dim3(B), dim3(256), 0, s, K, d_counts);
    hipLaunchKernelGGL(qf_root_assign, dim3(K.nchunk, B), dim3(AGT_SCAN_THREADS), 0, s, K, n, o.min_area, o.max_area);
    hipLaunchKernelGGL(qf_support, dim3(div_up(n, 256), B), dim3(256), 0, s, K, width, height);
    hipLaunchKernelGGL(qf_quads, dim3(div_up(K.maxc, 64), B), dim3(64), 0, s, K, d_counts, width, height, o.min_fill_pct);
    hipLaunchKernelGGL(qf_emit, dim3(B), dim3(256), 0, s, K, reinterpret_cast<uint32_t*>(d_quads), reinterpret_cast<uint32_t*>(d_records), d_counts);
    if (hipGetLastError() != hipSuccess) return AGT_QUADFIND_ERR_HIP;
    return AGT_QUADFIND_OK;
}

}  // extern "C"
