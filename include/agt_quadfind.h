/*
 * agt_quadfind.h -- C ABI of libagt_quadfind.so: the first stage of a tag detector on the MI355X (gfx950), "a quad is roughly here".
 * A frame is thresholded against its local contrast, its dark pixels are labelled into 4-connected components and every component
 * whose outline is close to a convex quadrilateral becomes a candidate quad.  The two later stages set what this one has to deliver:
 * agt_quad_refine (agt_quadfit.h) accepts seeds a few pixels off and gives the accuracy, agt_tag_decode (agt_tagcode.h) refuses
 * false candidates.  So this stage needs recall and roughly right corners, neither sub-pixel accuracy nor precision.
 *
 * The rule (fixed; tests/quad_detect_numpy.py states it independently).  All arithmetic is integer, int64 where products need it;
 * nothing depends on the order in which pixels are visited, so the device result equals the statement bit for bit.
 *   dark mask  tiles are 4 x 4 pixels, th = H / 4 by tw = W / 4 full tiles (integer division).  mn / mx = the smallest / largest
 *              pixel of a tile; MN / MX = the smallest mn / largest mx over the tile's 3 x 3 tile neighbourhood, clamped at the
 *              frame.  The tile of pixel (x, y) is (min(y / 4, th - 1), min(x / 4, tw - 1)).  The pixel of value v is dark iff
 *              MX - MN >= min_contrast and 2 v < MN + MX.
 *   components 4-connectivity over the dark pixels.  The label of a component is the smallest linear index y * W + x among its
 *              pixels; a pixel that is not dark has label -1.
 *   sums       per component: its area (pixels), its bounding box x0 y0 x1 y1 (inclusive) and for k = 0..15 the support point in
 *              direction d_k = (round(1024 cos(2 pi k / 16)), round(1024 sin(2 pi k / 16))), that is
 *              dx = 1024 946 724 392 0 -392 -724 -946 -1024 -946 -724 -392 0 392 724 946,
 *              dy = 0 392 724 946 1024 946 724 392 0 -392 -724 -946 -1024 -946 -724 -392:
 *              the pixel of the component that maximises x * dx + y * dy, ties to the smallest linear index.
 *   candidate  a component is a candidate when it passes, in this order:
 *              - min_area <= area <= max_area  (the components that pass this far are the ones `max_components` counts)
 *              - the bounding box touches no frame border: x0 > 0, y0 > 0, x1 < W - 1, y1 < H - 1
 *              - the 16 support points in k order with every element equal to its predecessor dropped, and the last dropped as
 *                well when it equals the first; while more than four remain, the vertex whose doubled triangle area with its two
 *                neighbours |(b - a) x (c - a)| (a before, c after b in the current cyclic list) is smallest is removed, ties to
 *                the lowest position in the current list.  Fewer than four left: no candidate
 *              - S2 = |sum_i x_i y_i+1 - x_i+1 y_i| (the doubled shoelace area of the four vertices) > 0
 *              - 200 * area >= min_fill_pct * S2   (the dark pixels fill at least min_fill_pct % of half the quadrilateral)
 *              - 20 * area <= 11 * S2 + 400        (and do not exceed it by more than a tenth plus a border's worth)
 *              - the four cross products of consecutive edges are all of one sign and non-zero
 *              - every squared edge length >= 64 (agt_quadfit.h's AGT_QUADFIT_MIN_EDGE, squared)
 *   corners    f32, per axis v + 0.5 * sign(4 v - the sum of the four vertices): pixel centres moved out to the outer edge of the
 *              border.  Exact in f32.  The vertices appear in surviving k order, which runs from +x towards +y: on a screen with y
 *              down that is clockwise.
 *   order      a frame's candidates come in ascending label order.  The component table holds the first `max_components`
 *              components inside the area limits in label order; the candidates are taken among those, and the first `max_quads`
 *              of them are written.  Either overflow sets a flag bit, writes nothing out of bounds and changes none of the
 *              candidates that are kept.
 *   counts     per frame four int32: dark components, components inside the area limits, candidates in the component table
 *              (before the max_quads cap), flag bits.
 *   outputs    entries of d_quads and d_records past a frame's count of written candidates are zero.
 * Limits that follow from the rule: 4-connectivity; a quiet zone under about 2 px merges a tag with its surroundings; a solid dark
 * region wider than about 16 px is hollow in the mask (its inner tiles see no contrast), which does not change its outline.
 *
 * Kernels: separate launches on the caller's stream.  None waits for another workgroup (no flag is spun on, no grid-wide barrier, no
 * persistent block); every loop has a bound the code shows; the union-find walks strictly decreasing indices and merges with
 * atomicMin.  The handle's workspace needs no clearing: every word a call reads it has written before.
 *
 * Conventions (those of agt_quadfit.h): every function returns 0 or a negative AGT_QUADFIND_ERR_*; nothing throws; every refusal comes
 * before any device work.  agt_quadfind_detect and agt_quadfind_labels take DEVICE pointers, enqueue on the given stream and return
 * without synchronising.  Two calls on one handle must be ordered by the caller (one stream, or events): they share the workspace.
 * A library of its own, separate from the per-frame library (include/agt_hip.h), which it neither needs nor changes.
 */
#ifndef AGT_QUADFIND_H
#define AGT_QUADFIND_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_QUADFIND_VERSION 100

#define AGT_QUADFIND_OK            0
#define AGT_QUADFIND_ERR_ARG     (-1)   /* NULL pointer where one is needed, a size or option outside the limits below */
#define AGT_QUADFIND_ERR_ALLOC   (-2)
#define AGT_QUADFIND_ERR_HIP     (-5)   /* a HIP runtime call failed */

#define AGT_QUADFIND_MIN_SIZE        8         /* width, height */
#define AGT_QUADFIND_MAX_SIZE        8192
#define AGT_QUADFIND_MAX_BATCH       64
#define AGT_QUADFIND_MAX_COMPONENTS  65536
#define AGT_QUADFIND_MAX_QUADS       65536     /* per frame, at most max_components */

#define AGT_QUADFIND_FLAG_QUADS       1        /* more candidates than max_quads: the first max_quads in label order were written */
#define AGT_QUADFIND_FLAG_COMPONENTS  2        /* more components inside the area limits than max_components: the first in label order were examined */

typedef struct agt_quadfind_options {   /* 16 bytes */
    int32_t min_contrast;    /* 1..255; default 40 */
    int32_t min_area;        /* >= 1; default 24 */
    int32_t max_area;        /* >= min_area; default INT32_MAX */
    int32_t min_fill_pct;    /* 0..100; default 5 */
} agt_quadfind_options;

typedef struct agt_quadfind_record {   /* 32 bytes */
    int32_t label, area, x0, y0, x1, y1;
    int64_t s2;
} agt_quadfind_record;

typedef struct agt_quadfind agt_quadfind;

int agt_quadfind_version(void);

/* The handle owns the workspace (tile minima and maxima, labels, areas, the component table) for frames of up to width x height and
 * batches of up to max_batch.  Limits: 8 <= width, height <= 8192, 1 <= max_batch <= 64, 1 <= max_quads <= max_components <= 65536. */
int agt_quadfind_create(int width, int height, int max_batch, int max_components, int max_quads, agt_quadfind** handle_out);
int agt_quadfind_destroy(agt_quadfind* handle);

/* Finds the candidate quads of B frames.  stream: a hipStream_t (NULL = the default stream).  d_frames: u8, frame b at
 * d_frames + b * frame_stride, rows `pitch` bytes apart.  options: HOST, NULL = the defaults.  d_quads: f32 [B][max_quads][4][2].
 * d_records: agt_quadfind_record [B][max_quads].  d_counts: i32 [B][4].
 * Limits: 8 <= width <= the handle's width, 8 <= height <= the handle's height, pitch >= width, frame_stride >= pitch * (height - 1)
 * + width when B > 1, 1 <= B <= max_batch, the options within the ranges above. */
int agt_quadfind_detect(agt_quadfind* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width,
                        int height, int B, const agt_quadfind_options* options, float* d_quads, agt_quadfind_record* d_records,
                        int32_t* d_counts);

/* The label image of the first two steps of the rule.  d_labels: i32 [B][height][width].  Same limits; 1 <= min_contrast <= 255. */
int agt_quadfind_labels(agt_quadfind* handle, void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width,
                        int height, int B, int min_contrast, int32_t* d_labels);

#ifdef __cplusplus
}
#endif
#endif
