/*
 * agt_tagcode.h -- C ABI of libagt_tagcode.so: the decode stage of a tag detector on the MI355X (gfx950).  Given quads (four image
 * points each, from the tracker's corner buffer or an outside detector) it reads the 6 x 6 payload printed inside each one, matches
 * it against a tag family and says which tag it is, how sure and whether the quad shows a tag at all.  Finding quads in an image is
 * NOT done here: that is agt_quadfind.h's job.
 *
 * The rule (fixed; tests/tag_decode_numpy.py states it independently).  Everything is FP64, f32 inputs are promoted exactly.
 *   quad       four image points q0..q3 (f32 pixels, integer coordinates at pixel centres) in the model's corner order, sitting at
 *              (u, v) = (-1,-1), (-1,+1), (+1,+1), (+1,-1): the outer edge of the black border.
 *   H          the homography from that square to the quad (closed-form square-to-quad map); x = H(u, v) is
 *              (H0 u + H1 v + H2, H3 u + H4 v + H5) / (H6 u + H7 v + H8).  H is written as computed, NOT normalised.
 *   cells      (r, c) with r, c in -1..8, centre u = (2c + 1) / 8 - 1, v = (2r + 1) / 8 - 1; the sample I(r, c) is the bilinear sample
 *              (1-a)(1-b) I00 + a(1-b) I10 + (1-a) b I01 + a b I11 of the u8 frame at H(u, v).
 *              ring: r or c in {-1, 8} (36 cells, the white quiet zone); border: r or c in {0, 7} inside the ring (28 cells, black);
 *              payload: r, c in 1..6 (36 cells).
 *   validity   decided before any address is formed from a coordinate:
 *              - all eight coordinates finite and at most AGT_TAGCODE_MAX_COORD in magnitude, else DEGENERATE
 *              - strictly convex: the four cross products of consecutive edges non-zero and of one sign, else DEGENERATE
 *              - at each of the 100 sample points the projective denominator non-zero and finite (and the point finite), else
 *                DEGENERATE; then 0 <= floor(x) <= w - 2 and 0 <= floor(y) <= h - 2 at every point, else OUTSIDE
 *   models     W(u, v) = a u + b v + c: the least-squares plane through the 36 ring samples; Bk the same through the 28 border samples
 *              (3 x 3 normal equations; both cell sets are symmetric about the centre, so the off-diagonal sums are exactly zero).
 *              At each payload cell thr = (W + Bk) / 2, d = I - thr, bit = d > 0.
 *              contrast = mean over the payload cells of W - Bk; contrast <= 0 is INVERTED.
 *              margin = min(mean of d over the 1-bits, mean of -d over the 0-bits); a class with no member contributes 0.
 *              For a clean tag the margin is half the local black / white contrast.  The scale is THIS RULE'S OWN: it is not the
 *              decision_margin of any apriltag release and thresholds do not carry over.
 *   word       bit 35 - (6 (r - 1) + (c - 1)) is the bit of payload cell (r, c): row-major, first cell in the highest bit
 *   match      for code i and k in 0..3 the candidate is the word of the code's bit matrix turned clockwise k times
 *              (np.rot90(bits_i, -k)); hamming = the smallest popcount(word XOR candidate), ties to the lowest i, then the lowest k.
 *              A quad in model order has rot = 0; the same quad with its points rolled by -k (np.roll(quad, -k, axis=0)) has rot = k.
 *              hamming > max_hamming is NO_MATCH; otherwise margin < min_margin is LOW_MARGIN; otherwise OK.
 *   precedence MASKED (mask byte 0), DEGENERATE, OUTSIDE, INVERTED, NO_MATCH, LOW_MARGIN, OK.
 *   record     id / hamming / rot carry the best match whenever a word was read (OK, NO_MATCH, LOW_MARGIN) and -1 otherwise;
 *              margin / contrast / word are 0 when no word was read.
 *   verdict    one byte per quad: status == OK, and when expected ids are given, id == expected[q] && rot == 0.
 *   H out      9 doubles per quad; zeros when the quad is MASKED or fails the coordinate or convexity checks.
 * One wave decodes one quad; every sum is a wave reduction in a fixed order, so two runs are bitwise equal.  No frame byte outside
 * [0, w) x [0, h) is read, whatever the coordinates.
 *
 * Conventions (those of agt_model.h): every function returns 0 or a negative AGT_TAGCODE_ERR_*; nothing throws; every refusal comes
 * before any device work.  agt_tag_decode takes DEVICE pointers, enqueues on the family's stream and returns without synchronising.
 * A library of its own, separate from the per-frame library (include/agt_hip.h), which it neither needs nor changes.
 */
#ifndef AGT_TAGCODE_H
#define AGT_TAGCODE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_TAGCODE_VERSION 100

#define AGT_TAGCODE_OK            0
#define AGT_TAGCODE_ERR_ARG     (-1)   /* NULL pointer (the family handle of agt_tag_decode excepted), a size or option outside the limits below */
#define AGT_TAGCODE_ERR_ALLOC   (-2)
#define AGT_TAGCODE_ERR_HIP     (-5)   /* a HIP runtime call failed */
#define AGT_TAGCODE_ERR_FAMILY (-13)   /* agt_tag_decode without a family handle; judged after every other argument */

#define AGT_TAGCODE_MAX_CODES   16384
#define AGT_TAGCODE_MAX_SIZE    16384      /* width, height (at least 4 each) */
#define AGT_TAGCODE_MAX_QUADS   1048576    /* B * Q per call */
#define AGT_TAGCODE_MAX_COORD   1048576.0  /* |coordinate| of a quad point, pixels: 64 x the largest frame */

/* status of a record, in order of precedence after MASKED */
#define AGT_TAG_OK          0
#define AGT_TAG_MASKED      1
#define AGT_TAG_DEGENERATE  2
#define AGT_TAG_OUTSIDE     3
#define AGT_TAG_INVERTED    4
#define AGT_TAG_NO_MATCH    5
#define AGT_TAG_LOW_MARGIN  6

typedef struct agt_tag_record {   /* 40 bytes */
    int32_t  id, hamming, rot, status;
    double   margin, contrast;
    uint64_t word;
} agt_tag_record;

typedef struct agt_tag_family agt_tag_family;

int agt_tagcode_version(void);

/* codes: n words (HOST), 1 <= n <= 16384, bit 35 - (6 r + c) = the bit of row r, column c of the 6 x 6 payload; bits_per_side must
 * be 6; a code with a bit above bit 35 is refused.  The four rotations are computed once here and uploaded.  stream: a hipStream_t
 * (NULL = the default stream); every agt_tag_decode of this family is enqueued on it.  The codes are not retained. */
int agt_tag_family_create(const uint64_t* codes, int n, int bits_per_side, void* stream, agt_tag_family** family_out);
int agt_tag_family_destroy(agt_tag_family* family);

/* Decodes B x Q quads.  d_frames: u8, frame b at d_frames + b * frame_stride, rows `pitch` bytes apart; the quads of batch entry b
 * are read in frame b.  d_quads: f32 [B][Q][4][2].  d_mask: u8 [B][Q] or NULL (all used).  d_expected: i32 [Q] or NULL.
 * d_records: agt_tag_record [B][Q].  d_ok: u8 [B][Q] verdicts or NULL.  d_corner_mask: u8 [B][4Q], each verdict four times -- the
 * corner mask agt_estimate_pose and agt_track_frame_detected take -- or NULL.  d_homography: f64 [B][Q][9] or NULL.
 * Limits: 4 <= width, height <= 16384, pitch >= width, frame_stride >= pitch * (height - 1) + width when B > 1, 1 <= B * Q <= 2^20,
 * 0 <= max_hamming <= 36, min_margin finite and >= 0. */
int agt_tag_decode(agt_tag_family* family, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int width, int height, int B,
                   const float* d_quads, const uint8_t* d_mask, int Q, const int32_t* d_expected, int max_hamming, double min_margin,
                   agt_tag_record* d_records, uint8_t* d_ok, uint8_t* d_corner_mask, double* d_homography);

#ifdef __cplusplus
}
#endif
#endif
