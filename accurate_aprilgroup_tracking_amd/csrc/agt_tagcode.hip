// libagt_tagcode.so (include/agt_tagcode.h): the decode stage of a tag detector.  One translation unit, one kernel.
//
// tag_decode_kernel: one wave per quad, TAG_WAVES waves per workgroup, no LDS, no atomics.
//   pass 1  lane l owns cell (l / 8, l % 8) of the 8 x 8 block: the 28 border cells and the 36 payload cells
//   pass 2  lanes 0..35 own the 36 ring cells (the quiet zone); the other lanes repeat cell 0 with weight 0
// Both passes' sample points are judged (ballots) before either forms an address.  The plane fits are 3 x 3 normal equations whose
// off-diagonal sums vanish exactly (both cell sets are symmetric about the centre), so each needs three data sums; every sum is an
// xor butterfly over the wave -- a fixed order, the same value in every lane.  The word is a ballot, the family search strides the
// lanes over the 4n candidates and ends in a wave minimum of (hamming << 16 | 4 i + k), which is the tie rule.
// Shared with the other image stages: the frame arguments and their rule (agt_side_frames.h), the family's device buffer
// (agt_side_buffers.h), the fixed-order wave sum and the bilinear fetch (agt_side_device.h).
#include <hip/hip_runtime.h>
#include <math.h>
#include <limits.h>
#include <stdint.h>
#include <new>
#include <vector>

#include "agt_side_buffers.h"
#include "agt_side_device.h"
#include "agt_side_frames.h"
#include "../../include/agt_tagcode.h"

#pragma clang fp contract(off)

static_assert(AGT_TAGCODE_OK == agt_side::OK && AGT_TAGCODE_ERR_ARG == agt_side::ERR_ARG && AGT_TAGCODE_ERR_ALLOC == agt_side::ERR_ALLOC &&
              AGT_TAGCODE_ERR_HIP == agt_side::ERR_HIP, "the codes of agt_side_math.h");

namespace {

using agt_side::Frames;

constexpr int TAG_WAVES = 4;            // quads per workgroup

struct TagCall {
    Frames F;
    int Q, total;
    const float* quads; const uint8_t* mask; const int32_t* expected;
    const uint64_t* cand; int n4;
    int max_hamming; double min_margin;
    agt_tag_record* rec; uint8_t* ok; uint8_t* cmask; double* H;
};

__host__ __device__ constexpr double cell_coord(int c) { return (2 * c + 1) / 8.0 - 1.0; }
// sum of u^2 over the ring cells (= the sum of v^2) and over the border cells
__host__ __device__ constexpr double ring_suu()
{
    double s = 0.0;
    for (int r = -1; r <= 8; r++) for (int c = -1; c <= 8; c++) if (r == -1 || r == 8 || c == -1 || c == 8) s += cell_coord(c) * cell_coord(c);
    return s;
}
__host__ __device__ constexpr double border_suu()
{
    double s = 0.0;
    for (int r = 0; r <= 7; r++) for (int c = 0; c <= 7; c++) if (r == 0 || r == 7 || c == 0 || c == 7) s += cell_coord(c) * cell_coord(c);
    return s;
}
constexpr double RING_SUU = ring_suu(), BORDER_SUU = border_suu(), RING_N = 36.0, BORDER_N = 28.0, PAYLOAD_N = 36.0;

__device__ __forceinline__ uint32_t wave_min(uint32_t x)
{
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) { uint32_t y = (uint32_t)__shfl_xor((int)x, m, 64); x = y < x ? y : x; }
    return x;
}

struct Sample { double x, y; bool degenerate, outside; };

__device__ __forceinline__ Sample sample_point(const double (&H)[9], double u, double v, int w, int h)
{
    Sample s;
    const double den = H[6] * u + H[7] * v + H[8];
    s.x = (H[0] * u + H[1] * v + H[2]) / den;
    s.y = (H[3] * u + H[4] * v + H[5]) / den;
    s.degenerate = !agt_finite(den) || den == 0.0 || !agt_finite(s.x) || !agt_finite(s.y);
    const double fx = floor(s.x), fy = floor(s.y);
    s.outside = !(fx >= 0.0 && fx <= (double)(w - 2) && fy >= 0.0 && fy <= (double)(h - 2));
    return s;
}

// only called for a point that passed sample_point's window: every address is inside [0, w) x [0, h)
__device__ __forceinline__ double bilinear(const uint8_t* __restrict__ img, size_t pitch, const Sample& s)
{
    const double fx = floor(s.x), fy = floor(s.y);
    return agt_bilinear_u8(img, pitch, (int)fx, (int)fy, s.x - fx, s.y - fy);
}

__global__ __launch_bounds__(64 * TAG_WAVES) void tag_decode_kernel(TagCall C)
{
    const int lane = threadIdx.x & 63;
    const int q = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * TAG_WAVES + (threadIdx.x >> 6)));
    if (q >= C.total) return;
    const int b = q / C.Q, qi = q - b * C.Q;

    int status = AGT_TAG_OK;
    double H[9];
#pragma unroll
    for (int i = 0; i < 9; i++) H[i] = 0.0;
    bool have_h = false;

    if (C.mask && C.mask[q] == 0) status = AGT_TAG_MASKED;
    if (status == AGT_TAG_OK) {
        const float* qp = C.quads + (size_t)q * 8;
        double x[4], y[4];
        bool fin = true;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            x[i] = (double)qp[2 * i]; y[i] = (double)qp[2 * i + 1];
            fin = fin && fabs(x[i]) <= AGT_TAGCODE_MAX_COORD && fabs(y[i]) <= AGT_TAGCODE_MAX_COORD;      // (NaN and inf fail)
        }
        bool pos = true, neg = true;
        if (fin) {
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const int j = (i + 1) & 3, k = (i + 2) & 3;
                const double cr = (x[j] - x[i]) * (y[k] - y[j]) - (y[j] - y[i]) * (x[k] - x[j]);
                pos = pos && cr > 0.0; neg = neg && cr < 0.0;
            }
        }
        if (!fin || !(pos || neg)) status = AGT_TAG_DEGENERATE;
        else {
            // unit square (s, t) -> quad with (0,0) q0, (1,0) q1, (1,1) q2, (0,1) q3; s = (v + 1) / 2, t = (u + 1) / 2
            const double dx1 = x[1] - x[2], dx2 = x[3] - x[2], sx = x[0] - x[1] + x[2] - x[3];
            const double dy1 = y[1] - y[2], dy2 = y[3] - y[2], sy = y[0] - y[1] + y[2] - y[3];
            const double det = dx1 * dy2 - dx2 * dy1;
            const double g = (sx * dy2 - dx2 * sy) / det, hh = (dx1 * sy - sx * dy1) / det;
            const double a = x[1] - x[0] + g * x[1], bb = x[3] - x[0] + hh * x[3];
            const double d = y[1] - y[0] + g * y[1], e = y[3] - y[0] + hh * y[3];
            H[0] = 0.5 * bb; H[1] = 0.5 * a; H[2] = 0.5 * (a + bb) + x[0];
            H[3] = 0.5 * e;  H[4] = 0.5 * d; H[5] = 0.5 * (d + e) + y[0];
            H[6] = 0.5 * hh; H[7] = 0.5 * g; H[8] = 0.5 * (g + hh) + 1.0;
            have_h = true;
        }
    }

    int id = -1, hamming = -1, rot = -1;
    double margin = 0.0, contrast = 0.0;
    uint64_t word = 0;

    if (status == AGT_TAG_OK) {
        // pass 1: the 8 x 8 block
        const int r1 = lane >> 3, c1 = lane & 7;
        const double u1 = cell_coord(c1), v1 = cell_coord(r1);
        const bool payload = r1 >= 1 && r1 <= 6 && c1 >= 1 && c1 <= 6;
        // pass 2: the ring, 10 + 10 cells of the rows r = -1 and r = 8, then 8 + 8 of the columns c = -1 and c = 8
        const bool ring = lane < 36;
        const int j = ring ? lane : 0;
        const int r2 = j < 10 ? -1 : j < 20 ? 8 : j < 28 ? j - 20 : j - 28;
        const int c2 = j < 10 ? j - 1 : j < 20 ? j - 11 : j < 28 ? -1 : 8;
        const double u2 = cell_coord(c2), v2 = cell_coord(r2);
        const Sample s1 = sample_point(H, u1, v1, C.F.w, C.F.h), s2 = sample_point(H, u2, v2, C.F.w, C.F.h);
        if (__ballot(s1.degenerate || s2.degenerate) != 0ull) status = AGT_TAG_DEGENERATE;
        else if (__ballot(s1.outside || s2.outside) != 0ull) status = AGT_TAG_OUTSIDE;
        else {
            const uint8_t* img = C.F.p + (size_t)b * C.F.stride;
            const double I1 = bilinear(img, C.F.pitch, s1), I2 = bilinear(img, C.F.pitch, s2);
            const double wb = payload ? 0.0 : 1.0, wr = ring ? 1.0 : 0.0;
            const double bk_a = agt_wave_sum_fixed(wb * u1 * I1) / BORDER_SUU, bk_b = agt_wave_sum_fixed(wb * v1 * I1) / BORDER_SUU, bk_c = agt_wave_sum_fixed(wb * I1) / BORDER_N;
            const double w_a = agt_wave_sum_fixed(wr * u2 * I2) / RING_SUU, w_b = agt_wave_sum_fixed(wr * v2 * I2) / RING_SUU, w_c = agt_wave_sum_fixed(wr * I2) / RING_N;
            const double Wv = w_a * u1 + w_b * v1 + w_c, Bv = bk_a * u1 + bk_b * v1 + bk_c;
            const double d = I1 - 0.5 * (Wv + Bv);
            const bool bit = payload && d > 0.0;
            const uint64_t ballot = __ballot(bit);
            contrast = agt_wave_sum_fixed(payload ? Wv - Bv : 0.0) / PAYLOAD_N;
            if (!(contrast > 0.0)) { status = AGT_TAG_INVERTED; contrast = 0.0; }
            else {
                const int n1 = __popcll(ballot), n0 = 36 - n1;
                const double s_hi = agt_wave_sum_fixed(bit ? d : 0.0), s_lo = agt_wave_sum_fixed(payload && !bit ? -d : 0.0);
                const double m1 = n1 ? s_hi / (double)n1 : 0.0, m0 = n0 ? s_lo / (double)n0 : 0.0;
                margin = m1 < m0 ? m1 : m0;
                // lane 8 r + c holds cell (r, c): reversed, row r's columns 1..6 sit at bits 62 - 8 r .. 57 - 8 r, column 1 highest
                const uint64_t rev = __brevll(ballot);
#pragma unroll
                for (int r = 1; r <= 6; r++) word |= ((rev >> (57 - 8 * r)) & 0x3Full) << (6 * (6 - r));
                uint32_t best = 0xFFFFFFFFu;
                for (int k = lane; k < C.n4; k += 64) {
                    const uint32_t key = ((uint32_t)__popcll(word ^ C.cand[k]) << 16) | (uint32_t)k;
                    best = key < best ? key : best;
                }
                best = wave_min(best);
                hamming = (int)(best >> 16); id = (int)((best & 0xFFFFu) >> 2); rot = (int)(best & 3u);
                if (hamming > C.max_hamming) status = AGT_TAG_NO_MATCH;
                else if (margin < C.min_margin) status = AGT_TAG_LOW_MARGIN;
            }
        }
    }

    if (lane == 0) {
        agt_tag_record rec;
        rec.id = id; rec.hamming = hamming; rec.rot = rot; rec.status = status;
        rec.margin = margin; rec.contrast = contrast; rec.word = word;
        C.rec[q] = rec;
        const uint8_t ok = status == AGT_TAG_OK && (!C.expected || (id == C.expected[qi] && rot == 0)) ? 1 : 0;
        if (C.ok) C.ok[q] = ok;
        if (C.cmask) {
#pragma unroll
            for (int i = 0; i < 4; i++) C.cmask[(size_t)q * 4 + i] = ok;
        }
        if (C.H) {
#pragma unroll
            for (int i = 0; i < 9; i++) C.H[(size_t)q * 9 + i] = have_h ? H[i] : 0.0;
        }
    }
}

// the word of the 6 x 6 bit matrix of `code` turned clockwise once: out[r][c] = in[5 - c][r]
uint64_t rotate_cw(uint64_t code)
{
    uint64_t out = 0;
    for (int r = 0; r < 6; r++)
        for (int c = 0; c < 6; c++)
            if ((code >> (35 - (6 * (5 - c) + r))) & 1ull) out |= 1ull << (35 - (6 * r + c));
    return out;
}

}  // namespace

struct agt_tag_family {
    AgtSideBuffers buf;     // (buf.stream: the stream of the decodes)
    uint64_t* d_cand;       // [n][4]: code i turned clockwise k times
    int n;
};

extern "C" {

int agt_tagcode_version(void) { return AGT_TAGCODE_VERSION; }

int agt_tag_family_destroy(agt_tag_family* f)
{
    return f ? agt_side_destroy(f) : AGT_TAGCODE_OK;
}

int agt_tag_family_create(const uint64_t* codes, int n, int bits_per_side, void* stream, agt_tag_family** out)
{
    if (!out) return AGT_TAGCODE_ERR_ARG;
    *out = nullptr;
    if (!codes || bits_per_side != 6 || n < 1 || n > AGT_TAGCODE_MAX_CODES) return AGT_TAGCODE_ERR_ARG;
    for (int i = 0; i < n; i++) if (codes[i] >> 36) return AGT_TAGCODE_ERR_ARG;
    std::vector<uint64_t> cand;
    try { cand.resize((size_t)n * 4); } catch (...) { return AGT_TAGCODE_ERR_ALLOC; }
    for (int i = 0; i < n; i++) {
        uint64_t w = codes[i];
        for (int k = 0; k < 4; k++) { cand[(size_t)i * 4 + k] = w; w = rotate_cw(w); }
    }
    agt_tag_family* f = new (std::nothrow) agt_tag_family();
    if (!f) return AGT_TAGCODE_ERR_ALLOC;
    f->buf.stream = (hipStream_t)stream; f->d_cand = nullptr; f->n = n;
    int rc = f->buf.alloc_n(&f->d_cand, cand.size());
    if (!rc) rc = f->buf.upload(f->d_cand, cand.data(), cand.size() * sizeof(uint64_t));
    if (rc) { agt_side_destroy(f); return rc; }
    *out = f;
    return AGT_TAGCODE_OK;
}

int agt_tag_decode(agt_tag_family* f, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height, int B,
                   const float* d_quads, const uint8_t* d_mask, int Q, const int32_t* d_expected, int max_hamming, double min_margin,
                   agt_tag_record* d_records, uint8_t* d_ok, uint8_t* d_corner_mask, double* d_homography)
{
    if (!agt_side::frames_ok(d_frames, pitch, frame_stride, width, height, 1, B, 4, AGT_TAGCODE_MAX_SIZE, AGT_TAGCODE_MAX_SIZE, INT_MAX)) return AGT_TAGCODE_ERR_ARG;
    if (!d_quads || !d_records) return AGT_TAGCODE_ERR_ARG;
    if (Q < 1 || (long long)B * (long long)Q > AGT_TAGCODE_MAX_QUADS) return AGT_TAGCODE_ERR_ARG;
    if (max_hamming < 0 || max_hamming > 36) return AGT_TAGCODE_ERR_ARG;
    if (!(min_margin >= 0.0) || !(min_margin <= 1.7976931348623157e308)) return AGT_TAGCODE_ERR_ARG;      // (NaN and inf fail)
    if (!f) return AGT_TAGCODE_ERR_FAMILY;

    TagCall C;
    C.F = Frames{ d_frames, pitch, frame_stride, width, height, B };
    C.Q = Q; C.total = B * Q;
    C.quads = d_quads; C.mask = d_mask; C.expected = d_expected;
    C.cand = f->d_cand; C.n4 = 4 * f->n;
    C.max_hamming = max_hamming; C.min_margin = min_margin;
    C.rec = d_records; C.ok = d_ok; C.cmask = d_corner_mask; C.H = d_homography;
    hipLaunchKernelGGL(tag_decode_kernel, dim3(agt_side::div_up(C.total, TAG_WAVES)), dim3(64 * TAG_WAVES), 0, f->buf.stream, C);
    if (hipGetLastError() != hipSuccess) return AGT_TAGCODE_ERR_HIP;
    return AGT_TAGCODE_OK;
}

}  // extern "C"
