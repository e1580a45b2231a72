/*
 * agt_chess.h -- C ABI of libagt_chess.so: the X-corners of a chessboard on the MI355X (gfx950), the pixel-level half of
 * findChessboardCorners.  A frame's corner response is computed, its local maxima become candidates and every candidate is refined to
 * its sub-pixel saddle point.  Putting the refined points into an nx x ny grid is host work over a few hundred points
 * (accurate_aprilgroup_tracking_amd/chessboard.py).
 *
 * The method is this project's own: a ring detector (the ChESS response of Bennett and Lasenby) and the saddle-point iteration behind
 * cv2.cornerSubPix.  It is NOT cv2's adaptive-threshold, erode and link-quads method; only the contract of the Python door is cv2's
 * (pattern size in, retval and (nx ny, 1, 2) float32 corners out, row by row).  No parity with cv2 is claimed.
 * The refinement is for X-corners of a chessboard only: an L-corner (a tag's corner) has no saddle point and is not refined this way.
 *
 * The rule (fixed; tests/chessboard_numpy.py states it independently).
 *   response   integer, int32.  The ring of pixel (x, y) is the 16 pixels (x + dx_k, y + dy_k), k = 0..15, at the rounded radius-5 offsets
 *              dx = 5 5 4 2 0 -2 -4 -5 -5 -5 -4 -2 0 2 4 5
 *              dy = 0 2 4 5 5 5 4 2 0 -2 -4 -5 -5 -5 -4 -2
 *              With the ring samples I_k:  SR = sum_{k<4} |I_k + I_{k+8} - I_{k+4} - I_{k+12}|,  DR = sum_{k<8} |I_k - I_{k+8}|,
 *              L = the centre pixel plus its four 4-neighbours, S = the ring sum,
 *              R = 5 (SR - DR) - |5 S - 16 L|
 *              (five times the ChESS response, the mean term kept exact).  A pixel closer than 5 to a frame border has R = 0.
 *   candidate  Rmax = the frame's largest response (at least 0: the border pixels).  Pixel i = y W + x is a candidate iff
 *              R >= min_response, 100 R >= rel_pct Rmax, and over its (2 nms + 1)^2 neighbourhood clamped at the frame R is strictly
 *              greater than the response of every pixel of smaller linear index and greater than or equal to that of every pixel of
 *              larger linear index (ties go to the smallest linear index).
 *   order      a frame's candidates come in raster order (ascending linear index).  The first max_candidates are written, three int32
 *              each: x, y, R; the entries behind them are zero.  More candidates than that set AGT_CHESS_FLAG_CANDIDATES, write nothing
 *              out of bounds and change no candidate that is kept.
 *   counts     per frame four int32: candidates (before the cap), candidates written, Rmax, flag bits.
 *   refine     FP64, nothing contracted.  n = 2 half + 1; the weights are w_i = exp(-((i - half) / half)^2), i = 0..n-1, evaluated on the
 *              host.  The estimate q starts at the seed (x, y).  Each of `iters` iterations, in this order:
 *              - with (X, Y) = floor(q) per axis: the window fits iff X - half - 1 >= 0, Y - half - 1 >= 0, X + half + 2 <= W - 1 and
 *                Y + half + 2 <= H - 1.  If not: verdict BORDER, stop.  No byte outside the image is ever read.
 *              - samples s[r][c], r, c = 0..n+1, at (q.x + c - half - 1, q.y + r - half - 1): with a = q.x - X, b = q.y - Y and the
 *                pixels i00 i10 / i01 i11 at (X + c - half - 1, Y + r - half - 1) and its right, lower and lower-right neighbours
 *                s = (1 - a)(1 - b) i00 + a (1 - b) i10 + (1 - a) b i01 + a b i11, evaluated left to right
 *              - term t = i n + j (i the row, j the column of the window, 0..n-1): gx = 0.5 (s[i+1][j+2] - s[i+1][j]),
 *                gy = 0.5 (s[i+2][j+1] - s[i][j+1]), m = w_i w_j, px = j - half, py = i - half,
 *                gxx = gx gx m, gxy = gx gy m, gyy = gy gy m, and the five addends gxx, gxy, gyy, gxx px + gxy py, gxy px + gyy py
 *              - each of the five sums (a, b, c, b1, b2) in this fixed order: partial P[t mod 64] takes its terms in ascending t, starting
 *                from 0.0; then for m = 32, 16, 8, 4, 2, 1 every P[l] becomes P[l] + P[l xor m] (all at once); the sum is P[0]
 *              - det = a c - b b.  If not det > min_det (NaN included): verdict FLAT, stop.
 *              - q = q + ((c b1 - b b2) / det, (a b2 - b b1) / det);  d = q - seed, shift = sqrt(d.x d.x + d.y d.y).
 *                If not shift <= max_shift: verdict SHIFT, stop.
 *              Verdict OK after the last iteration.  The record holds q (f64, and rounded to f32), the last det and shift computed (0
 *              when none was) and the verdict; a candidate whose verdict is not OK keeps its seed coordinates.
 *              Records behind a frame's written candidates are zero.
 *
 * Kernels: separate launches on the caller's stream.  None waits for another workgroup (no flag is spun on, no grid-wide barrier, no
 * persistent block); every loop has a bound the code shows.  The handle's workspace needs no clearing: every word a call reads it has
 * written before.  Nothing depends on the order in which pixels or candidates are visited: two runs give the same bits.
 *
 * Conventions (those of agt_quadfind.h): every function returns 0 or a negative AGT_CHESS_ERR_*; nothing throws; every refusal comes
 * before any device work.  The calls take DEVICE pointers, enqueue on the given stream and return without synchronising.  Two calls on
 * one handle must be ordered by the caller (one stream, or events): they share the workspace.  A library of its own, separate from the
 * per-frame library (include/agt_hip.h), which it neither needs nor changes.
 */
#ifndef AGT_CHESS_H
#define AGT_CHESS_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_CHESS_VERSION 100

#define AGT_CHESS_OK            0
#define AGT_CHESS_ERR_ARG     (-1)   /* NULL pointer where one is needed, a size or option outside the limits below */
#define AGT_CHESS_ERR_ALLOC   (-2)
#define AGT_CHESS_ERR_HIP     (-5)   /* a HIP runtime call failed */

#define AGT_CHESS_MIN_SIZE        11        /* width, height: one pixel with a ring */
#define AGT_CHESS_MAX_SIZE        8192
#define AGT_CHESS_MAX_BATCH       64
#define AGT_CHESS_MAX_CANDIDATES  65536     /* per frame */
#define AGT_CHESS_MAX_NMS         8
#define AGT_CHESS_MAX_HALF        11        /* the reference's cornerSubPix window */
#define AGT_CHESS_MAX_ITERS       64

#define AGT_CHESS_FLAG_CANDIDATES 1         /* more candidates than max_candidates: the first in raster order were written */

#define AGT_CHESS_VERDICT_OK      0
#define AGT_CHESS_VERDICT_BORDER  1         /* the window left the frame */
#define AGT_CHESS_VERDICT_FLAT    2         /* det <= min_det or not a number */
#define AGT_CHESS_VERDICT_SHIFT   3         /* the estimate left max_shift pixels from the seed */

typedef struct agt_chess_options {   /* 40 bytes */
    int32_t min_response;    /* 1..INT32_MAX; default 200 */
    int32_t rel_pct;         /* 0..100; default 10 */
    int32_t nms;             /* 1..AGT_CHESS_MAX_NMS; default 3 */
    int32_t half;            /* 1..AGT_CHESS_MAX_HALF; default 5 */
    int32_t iters;           /* 1..AGT_CHESS_MAX_ITERS; default 10 */
    int32_t reserved0;       /* 0 */
    double  max_shift;       /* > 0, at most 64; default 3.0 (pixels) */
    double  min_det;         /* >= 0, finite; default 1.0 ((gray / px)^4, summed over the weighted window) */
} agt_chess_options;

typedef struct agt_chess_record {   /* 48 bytes */
    double  x, y;            /* the refined point (the seed when the verdict is not OK) */
    double  det, shift;
    float   xf, yf;          /* (float)x, (float)y: the corner list's entry */
    uint8_t verdict;         /* AGT_CHESS_VERDICT_* */
    uint8_t reserved[7];     /* 0 */
} agt_chess_record;

typedef struct agt_chess agt_chess;

int agt_chess_version(void);

/* The handle owns the workspace (the response image, the candidate mask, the scan's counts) for frames of up to width x height and
 * batches of up to max_batch.  Limits: 11 <= width, height <= 8192, 1 <= max_batch <= 64, 1 <= max_candidates <= 65536. */
int agt_chess_create(int width, int height, int max_batch, int max_candidates, agt_chess** handle_out);
int agt_chess_destroy(agt_chess* handle);

/* The response image of B frames.  stream: a hipStream_t (NULL = the default stream).  d_frames: u8, frame b at d_frames + b *
 * frame_stride, rows `pitch` bytes apart.  d_response: i32 [B][height][width].
 * Limits: 11 <= width <= the handle's width, 11 <= height <= the handle's height, pitch >= width, frame_stride >= pitch * (height - 1)
 * + width when B > 1, 1 <= B <= max_batch. */
int agt_chess_response(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                       int B, int32_t* d_response);

/* Response and candidates.  options: HOST, NULL = the defaults (min_response, rel_pct and nms are used; all are checked).
 * d_candidates: i32 [B][max_candidates][3].  d_counts: i32 [B][4].  Same limits, the options within the ranges above. */
int agt_chess_candidates(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                         int B, const agt_chess_options* options, int32_t* d_candidates, int32_t* d_counts);

/* Refines given seeds: d_candidates and d_counts as agt_chess_candidates writes them (x, y of each entry and counts[b][1] are read;
 * a count is clamped to 0..max_candidates, a seed anywhere is safe: its window is checked).  d_records: agt_chess_record
 * [B][max_candidates].  half, iters, max_shift and min_det are used; all options are checked. */
int agt_chess_refine(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                     int B, const agt_chess_options* options, const int32_t* d_candidates, const int32_t* d_counts,
                     agt_chess_record* d_records);

/* agt_chess_candidates, then agt_chess_refine on what it found. */
int agt_chess_corners(agt_chess* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height,
                      int B, const agt_chess_options* options, int32_t* d_candidates, int32_t* d_counts, agt_chess_record* d_records);

#ifdef __cplusplus
}
#endif
#endif
