/*
 * agt_quadfit.h -- C ABI of libagt_quadfit.so: the edge refinement stage of a tag detector on the MI355X (gfx950).  Given quads that
 * are roughly right (the tracker's corner buffer, re-projected corners, an outside detector's candidates) it fits a line to the
 * black-to-white step along each of the four border edges and intersects the lines: the quad snapped onto the tag's border, with a
 * strength that tells a tag's border from background.  Finding quads without a seed is NOT done here (agt_quadfind.h).  No window around a corner is
 * iterated (a tag corner is an L-corner, not a saddle): whole edges are fitted and a corner comes out only as the intersection of two
 * fitted lines.
 *
 * The rule (fixed; tests/quad_refine_numpy.py states it independently).  Everything is FP64, f32 inputs are promoted exactly; only
 * + - * / sqrt, comparisons and floor are used.
 *   quad       four image points q0..q3 as in agt_tagcode.h: f32 pixels, integer coordinates at pixel centres, on the outer edge of the
 *              black border, either orientation.  sg = +1 when the shoelace sum  sum_e (x_e y_e+1 - x_e+1 y_e)  is positive, else -1.
 *              The tag is black inside its outer edge and has a white quiet zone outside it.
 *   validity   decided before any address is formed from a coordinate:
 *              - all eight coordinates finite and at most AGT_QUADFIT_MAX_COORD in magnitude, and the quad strictly convex (the four
 *                cross products of consecutive edges non-zero and of one sign), else DEGENERATE
 *              - every edge at least AGT_QUADFIT_MIN_EDGE px long, else SHORT
 *   one pass   all four edges are computed from the same iterate (Jacobi).  Edge e runs from a = q_e to b = q_e+1:
 *              d = b - a, L = sqrt(dx dx + dy dy), outward normal n = sg (dy, -dx) / L, search half-width r = min(range_px, L / 8)
 *              (at most one cell of the tag).
 *              16 stations i = 0..15 at u_i = ((i + 0.5) / 16 - 0.5) 0.75 (the middle three quarters), p_i = a + (u_i + 0.5) d.
 *              17 offsets o_k = r k / 8, k = -8..8.  At each,  dg = I(p_i + (o_k + 1) n) - I(p_i + (o_k - 1) n)  with I the bilinear
 *              sample of agt_tagcode.h: the gradient along the normal over a fixed baseline of 1 px to either side.
 *              A station is DROPPED when any of its 34 sample points is not finite or fails 0 <= floor(x) <= w - 2,
 *              0 <= floor(y) <= h - 2.  Offsets with dg <= 0 contribute nothing (the wrong polarity: the payload side of the border, or
 *              the far side of the quiet zone).  Mc = sum dg^2, Mn = sum dg^2 o_k, gm = max dg (0 when no dg is positive).
 *              A station is USED when it was not dropped and Mc > 0; its offset is o_i = Mn / Mc.
 *              Edge fit, unweighted over the used stations: o(u) = alpha + beta u by the 2 x 2 normal equations
 *              (s0 = sum 1, s1 = sum u, s2 = sum u^2, y0 = sum o, y1 = sum o u; det = s0 s2 - s1 s1,
 *              alpha = (s2 y0 - s1 y1) / det, beta = (s0 y1 - s1 y0) / det).
 *              The fitted line runs through P0 = a + (alpha - beta / 2) n and P1 = b + (alpha + beta / 2) n.
 *              Edge strength = the mean of gm over the used stations (0 with none); edge residual = the rms of o_i - o(u_i).
 *              Fewer than 8 used stations on any edge: WEAK.
 *              New corner e = the intersection of line e-1 and line e in the two-point cross-product form, taken about q_e (the four
 *              points minus q_e, the result plus q_e): d0 = P1' - P0', d1 = P1 - P0, den = d0x d1y - d0y d1x,
 *              c0 = P0'x P1'y - P0'y P1'x, c1 likewise, x = (d0x c1 - c0 d1x) / den, y = (d0y c1 - c0 d1y) / den.
 *              |den| <= 1e-12 |d0| |d1| (or not comparable): DIVERGED.
 *   iterations exactly `iters` passes; each starts from the corners of the one before, with L, n and r computed anew (sg is the input's).
 *   verdict    after the last pass: corners not finite, or no longer strictly convex with the input's orientation: DIVERGED;
 *              shift = max_e |q_out,e - q_in,e| > 2 range_px: DIVERGED;  strength = the smallest edge strength of the last pass
 *              < min_strength: WEAK.
 *   precedence MASKED (mask byte 0), DEGENERATE, SHORT, WEAK, DIVERGED, OK: a pass that refuses with DIVERGED, or a final quad that
 *              would be DIVERGED, is WEAK when its strength is below min_strength.
 *   record     passes = the passes completed (four lines fitted and intersected).  strength = the smallest edge strength of the last
 *              pass begun, resid = the largest edge residual of the last pass that fitted four lines, shift as above whenever the
 *              final corners are finite; each 0 if never computed.
 *   outputs    for any status but OK the output corners are the input corners bit for bit (f64: promoted); otherwise the refined
 *              corners, the f32 ones rounded once from f64.  The verdict byte is status == OK.
 * A tag's border is a step of the full black / white contrast (strength above 100 for the renderer's 30 / 225), background texture
 * stays an order of magnitude below: the default min_strength of the Python doors (40) lies between.  With cells under two pixels the
 * 1-px baseline reaches the next cell boundary and biases the fit (a third of a pixel at 1.4-px cells); a tag corner is otherwise found
 * to about a tenth of a pixel from a seed 1 px off.
 * One wave refines one quad; every sum is a reduction in a fixed order, so two runs are bitwise equal.  No frame byte outside
 * [0, w) x [0, h) is read, whatever the coordinates.
 *
 * Conventions (those of agt_tagcode.h): every function returns 0 or a negative AGT_QUADFIT_ERR_*; nothing throws; every refusal comes
 * before any device work.  agt_quad_refine takes DEVICE pointers, enqueues on the given stream and returns without synchronising.
 * There is no handle: the rule needs no table.  A library of its own, separate from the per-frame library (include/agt_hip.h).
 */
#ifndef AGT_QUADFIT_H
#define AGT_QUADFIT_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_QUADFIT_VERSION 100

#define AGT_QUADFIT_OK            0
#define AGT_QUADFIT_ERR_ARG     (-1)   /* NULL pointer where one is needed, a size or option outside the limits below */
#define AGT_QUADFIT_ERR_HIP     (-5)   /* a HIP runtime call failed */

#define AGT_QUADFIT_MAX_SIZE    16384      /* width, height (at least 4 each) */
#define AGT_QUADFIT_MAX_QUADS   1048576    /* B * Q per call */
#define AGT_QUADFIT_MAX_COORD   1048576.0  /* |coordinate| of a quad point, pixels: 64 x the largest frame */
#define AGT_QUADFIT_MIN_EDGE    8.0        /* shortest edge fitted, pixels */
#define AGT_QUADFIT_MAX_RANGE   16.0       /* largest range_px */
#define AGT_QUADFIT_MAX_ITERS   8

/* status of a record, in order of precedence after MASKED */
#define AGT_QUAD_OK          0
#define AGT_QUAD_MASKED      1
#define AGT_QUAD_DEGENERATE  2
#define AGT_QUAD_SHORT       3
#define AGT_QUAD_WEAK        4
#define AGT_QUAD_DIVERGED    5

typedef struct agt_quad_record {   /* 32 bytes */
    int32_t status, passes;
    double  strength, shift, resid;
} agt_quad_record;

int agt_quadfit_version(void);

/* Refines B x Q quads.  stream: a hipStream_t (NULL = the default stream).  d_frames: u8, frame b at d_frames + b * frame_stride, rows
 * `pitch` bytes apart; the quads of batch entry b are read in frame b.  d_quads: f32 [B][Q][4][2].  d_mask: u8 [B][Q] or NULL (all
 * used).  d_quads_out: f32 [B][Q][4][2].  d_quads64_out: f64 [B][Q][4][2] or NULL.  d_records: agt_quad_record [B][Q].  d_ok: u8 [B][Q]
 * verdicts or NULL.  d_corner_mask: u8 [B][4Q], each verdict four times -- the corner mask agt_estimate_pose and
 * agt_track_frame_detected take -- or NULL.  The outputs must not overlap the inputs.
 * Limits: 4 <= width, height <= 16384, pitch >= width, frame_stride >= pitch * (height - 1) + width when B > 1, 1 <= B * Q <= 2^20,
 * 0 < range_px <= 16 finite, 1 <= iters <= 8, min_strength finite and >= 0. */
int agt_quad_refine(void* stream, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height, int B,
                    const float* d_quads, const uint8_t* d_mask, int Q, double range_px, int iters, double min_strength,
                    float* d_quads_out, double* d_quads64_out, agt_quad_record* d_records, uint8_t* d_ok, uint8_t* d_corner_mask);

#ifdef __cplusplus
}
#endif
#endif
