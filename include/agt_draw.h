/*
 * agt_draw.h -- C ABI of libagt_draw.so: the output stage of the per-frame loop on the MI355X (gfx950).  The reference ends every
 * frame in two images: the camera frame with a dot on every projected model corner, and a black frame with the tag outlines of the
 * body (detect_pose.py:441-465, draw.py:63-153).  This library paints both where the frames and the pose already are: in HBM.
 * agt_draw_pose_lists turns projected points into two display lists without the pose coming back to the host, agt_draw_raster paints
 * a display list into a batch of frames.  Text (putText), filled contours, capture and windows are NOT done here.
 *
 * Drawing is binary: a pixel is painted with the primitive's colour or left alone.  cv.LINE_AA and cv2's exact circle and line
 * rasters are not reproduced (cv2 is not part of this project and nothing here pins them); the rule below is this library's own,
 * as DESIGN.md section 2 says of the rest.
 *
 * The rule (fixed; integers only; tests/overlay_numpy.py states it independently).
 *   primitive  agt_draw_prim, 32 bytes: kind, x0, y0, x1, y1, size, colour B G R and one unused byte.  Integer coordinates are pixel
 *              centres.  A display list is agt_draw_prim [B][P]: the primitives of entry b are painted into frame b in list order, a
 *              later primitive paints over an earlier one.
 *   validity   decided before any address is formed.  A primitive paints nothing when its kind is not DISC or SEGMENT (NONE is the
 *              kind that is meant to paint nothing), when any of x0, y0, x1, y1 -- all four, whatever the kind -- exceeds
 *              AGT_DRAW_MAX_COORD in magnitude, or when its size is outside 0..AGT_DRAW_MAX_SIZE.  The rest of the list is painted
 *              as if the primitive were not there.
 *   disc       centre c = (x0, y0), radius r = size (x1, y1 are judged for validity and otherwise unused).  Pixel p is painted iff
 *              dx^2 + dy^2 <= r^2 + r  with (dx, dy) = p - c.  r = 0 is the centre pixel; r = 5 gives rows of
 *              5, 7, 9, 11, 11, 11, 11, 11, 9, 7, 5 pixels, 97 in all.
 *   segment    from a = (x0, y0) to b = (x1, y1), thickness T = size.  d = b - a, L2 = d.d, t = (p - a).d.  Pixel p is painted
 *              if t <= 0:          iff 4 |p - a|^2 <= T^2
 *              else if t >= L2:    iff 4 |p - b|^2 <= T^2
 *              else:               iff 4 (dx (py - ay) - dy (px - ax))^2 <= T^2 L2
 *              -- the pixels within T / 2 of the segment, with round caps.  a == b always takes the first branch (21 pixels for
 *              T = 5).  T = 1 leaves no gap in any direction.  An odd T on a horizontal or vertical segment paints exactly T rows
 *              (columns); an EVEN T paints T + 1 (the pixels at distance exactly T / 2 on either side belong to it).  T = 0 paints
 *              the pixels that lie exactly on the segment.
 *   no overflow  with coordinates up to 32767 in magnitude and pixels below 16384 every term above fits 64 bits except the square of
 *              the cross product (|cross| reaches 2^33).  T^2 L2 stays below 2^46, so a pixel with |cross| > 2^22 is outside
 *              before anything is squared, and for the others 4 cross^2 <= 2^46: the kernel decides exactly the predicate above.
 *   frames     u8, `channels` 1 or 3 interleaved.  A painted pixel takes colour[0..2] (1 channel: colour[0]); painting is in place and
 *              opaque.  With AGT_DRAW_CLEAR every pixel that no primitive covers is written 0 -- the black drawing frame without a
 *              separate fill.  Without it such a pixel is not written at all.
 * The raster gathers: a workgroup owns a tile of pixels, tests the bounding boxes of the list against its tile in chunks of
 * AGT_DRAW_CHUNK primitives, keeps the survivors of a chunk in LDS in list order, and every pixel walks that short list (last chunk
 * first, last survivor first: the first hit is the one that shows) and is written at most once, by one thread.  No atomics, no
 * workgroup waits for another, every loop is bounded; the result does not depend on tile shape or chunk size, so two runs are
 * bitwise equal.  No byte outside [0, width * channels) x [0, height) of a frame is read or written, whatever the coordinates.
 *
 * The pose lists (agt_draw_pose_lists): points [B][n][2], f32 (promoted exactly) or f64.
 *   gate       entry b is drawn when d_gate is NULL or d_gate[b * gate_stride] == 1.0 (pass the state records' AGT_ST_OK with stride
 *              AGT_STATE_STRIDE: the reference draws an accepted pose only); otherwise both lists of entry b are all NONE.
 *   dots       point i -> DISC at (rint(x), rint(y)), rounded half to even as np.round does, size = radius, x1 = x0, y1 = y0.  Drawn
 *              when both coordinates are finite and the ROUNDED values satisfy 0 <= x < width, 0 <= y < height, as draw.py:144-151
 *              judges them (-0.4 rounds to 0 and is drawn, width - 0.5 rounds to an even width and is not); otherwise NONE.  The
 *              reference hard-codes 1280 x 720 there; here it is the frame's size.
 *   outline    every group of corners_per_tag = 4 points a, b, c, d is truncated toward zero as int() does.  If any of the four is
 *              not finite or its truncated value lies outside 0 <= x < width, 0 <= y < height, the group's four entries are NONE
 *              (draw.py:88-99); otherwise they are the SEGMENTs a->b, b->c, c->d, d->a with size = thickness.
 *   a NONE entry is 32 zero bytes; the unused colour byte of every entry is 0.
 *
 * Conventions (those of agt_quadfit.h): every function returns 0 or a negative AGT_DRAW_ERR_*; nothing throws; every refusal comes
 * before any device work.  The functions take DEVICE pointers, enqueue on the given stream and return without synchronising.  There
 * is no handle.  A library of its own, separate from the per-frame library (include/agt_hip.h).
 */
#ifndef AGT_DRAW_H
#define AGT_DRAW_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_DRAW_VERSION 100

#define AGT_DRAW_OK            0
#define AGT_DRAW_ERR_ARG     (-1)   /* NULL pointer where one is needed, a size or option outside the limits below */
#define AGT_DRAW_ERR_HIP     (-5)   /* a HIP runtime call failed */

#define AGT_DRAW_MAX_SIZE_PX   16384     /* width, height (at least 1 each) */
#define AGT_DRAW_MAX_PRIMS     4096      /* P: primitives per frame */
#define AGT_DRAW_MAX_TOTAL     1048576   /* B * P per call */
#define AGT_DRAW_MAX_POINTS    4096      /* n of agt_draw_pose_lists (a multiple of 4, at least 4) */
#define AGT_DRAW_MAX_COORD     32767     /* |x0|, |y0|, |x1|, |y1| of a primitive that paints */
#define AGT_DRAW_MAX_SIZE      64        /* radius of a disc, thickness of a segment */
#define AGT_DRAW_CHUNK         256       /* primitives tested per pass of a tile: the survivors' LDS is AGT_DRAW_CHUNK records */

/* kind */
#define AGT_DRAW_NONE     0
#define AGT_DRAW_DISC     1
#define AGT_DRAW_SEGMENT  2

/* flags of agt_draw_raster */
#define AGT_DRAW_CLEAR    1   /* write 0 to every pixel no primitive covers */

/* dtype of agt_draw_pose_lists */
#define AGT_DRAW_F32      0
#define AGT_DRAW_F64      1

typedef struct agt_draw_prim {   /* 32 bytes */
    int32_t kind;
    int32_t x0, y0, x1, y1;
    int32_t size;
    uint8_t color[4];            /* B, G, R, unused */
    int32_t reserved;            /* pads the record to 32 bytes; not read */
} agt_draw_prim;

int agt_draw_version(void);

/* Paints display lists into frames.  stream: a hipStream_t (NULL = the default stream).  d_frames: u8, frame b at
 * d_frames + b * frame_stride, rows `pitch` bytes apart, `channels` interleaved bytes per pixel.  d_prims: agt_draw_prim [B][P]; may be
 * NULL only when P = 0.  flags: 0 or AGT_DRAW_CLEAR.  The list must not overlap the frames.
 * Limits: 1 <= width, height <= 16384, channels 1 or 3, pitch >= width * channels,
 * frame_stride >= pitch * (height - 1) + width * channels when B > 1, 0 <= P <= 4096, 1 <= B, B * P <= 2^20.
 * With P = 0 and no AGT_DRAW_CLEAR nothing is launched. */
int agt_draw_raster(void* stream, uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height, int channels, int B,
                    const agt_draw_prim* d_prims, int P, unsigned flags);

/* Builds the reference's two display lists from projected points (see above).  d_points: [B][n][2] of `dtype` (AGT_DRAW_F32 /
 * AGT_DRAW_F64).  d_gate: f64, entry b at d_gate[b * gate_stride], or NULL (all drawn).  dot_color / line_color: B | G << 8 | R << 16.
 * d_dots, d_outline: agt_draw_prim [B][n] each; every entry is written.  The outputs must not overlap the inputs or each other.
 * Limits: n a multiple of 4 with 4 <= n <= 4096, 1 <= B with B * n <= 2^20, 1 <= width, height <= 16384, corners_per_tag == 4,
 * radius and thickness in 0..64, gate_stride >= 1 when d_gate is given, the colours below 2^24. */
int agt_draw_pose_lists(void* stream, const void* d_points, int dtype, int n, int B, const double* d_gate, size_t gate_stride,
                        int width, int height, int corners_per_tag, int radius, int thickness, uint32_t dot_color, uint32_t line_color,
                        agt_draw_prim* d_dots, agt_draw_prim* d_outline);

#ifdef __cplusplus
}
#endif
#endif
