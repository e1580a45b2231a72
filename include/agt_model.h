/*
 * agt_model.h -- C ABI of libagt_model.so: the dense model's template learned from a recording on the MI355X (gfx950).
 *
 * The dense photometric stage (agt_dense_refine, agt_tracker_dense of include/agt_hip.h) minimises I~(project(X_i; p)) - T_i; the
 * samples X_i and the template T_i are the caller's.  This library makes T from frames with known poses.
 *
 * The rule (fixed; tests/dense_model_numpy.py states it independently).  Everything is FP64, f32 inputs are promoted exactly.
 *   An observation of sample i in frame f exists iff
 *     1. use_f != 0
 *     2. tag_i is visible under p_f by the rule of agt_tracker_visibility (include/agt_hip.h): c_o = the mean of the tag's four
 *        corners summed in index order, n_o = facing (p3 - p0) x (p1 - p0), visible iff c_c.z > 0 and cos > cos(max_view_deg)
 *     3. the sample's own camera-frame z > 0
 *     4. (u, v) = project(camera, p_f, X_i) lies in the dense stage's validity window: 1 <= floor(u) <= w - 3, 1 <= floor(v) <= h - 3
 *   and its value is the bilinear sample  I = (1-a)(1-b) I00 + a(1-b) I10 + (1-a) b I01 + a b I11.
 *   Plain pass: per sample, in frame order over the whole pass: n += 1, S += I, S2 += I * I.
 *   Clipped pass (clip_sigma > 0, sigma_floor >= 0, reference = the finished previous pass): mean_r = S_r / n_r,
 *     std_r = sqrt(max(S2_r / n_r - mean_r^2, 0)); an observation of a sample with n_r > 0 counts iff
 *     |I - mean_r| <= clip_sigma * max(std_r, sigma_floor), otherwise rejected += 1; a sample with n_r = 0 takes every observation.
 *   frame_obs[f] = the observations counted in frame f.
 * A thread owns a sample and adds its frames in order, so the sums of a pass depend on the frames and their order only -- not on how
 * the recording was cut into calls -- and two runs are bitwise equal.
 *
 * Conventions: every function returns 0 or a negative AGT_MODEL_ERR_*; nothing throws.  The calls are synchronous; poses are HOST
 * arrays of 6 doubles (rvec, tvec), frames are DEVICE memory.  A handle is not re-entrant.
 * An offline tool, separate from the per-frame library (include/agt_hip.h), which it neither needs nor changes.
 */
#ifndef AGT_MODEL_H
#define AGT_MODEL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_MODEL_VERSION 100

#define AGT_MODEL_OK            0
#define AGT_MODEL_ERR_ARG     (-1)   /* NULL pointer, a size outside the limits, sample_tag out of range, max_view_deg outside (0, 90],
                                        facing not +-1, pitch < width, count outside 1..4096, a used pose that is not finite,
                                        a negative or non-finite clip_sigma / sigma_floor */
#define AGT_MODEL_ERR_ALLOC   (-2)
#define AGT_MODEL_ERR_CAMERA  (-3)   /* unknown camera model: distortion count not in {0,4,5,8,12,14} */
#define AGT_MODEL_ERR_HIP     (-5)   /* a HIP runtime call failed */
#define AGT_MODEL_ERR_ORDER   (-12)  /* accumulate or read before begin_pass; a clipped pass without a reference pass */

#define AGT_MODEL_MAX_TAGS     256
#define AGT_MODEL_MAX_SAMPLES  4194304
#define AGT_MODEL_MAX_SIZE     16384   /* width, height (at least 4 each) */
#define AGT_MODEL_MAX_COUNT    4096    /* frames per accumulate call */

typedef struct agt_model_problem {
    const double*  K;             /* 3 x 3 row-major camera matrix */
    const double*  dist;          /* ndist distortion coefficients (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tau_x tau_y), NULL when ndist = 0 */
    int32_t        ndist;         /* 0, 4, 5, 8, 12 or 14 */
    int32_t        width, height; /* of every frame */
    int32_t        n_tags;        /* 1 <= T <= 256 */
    const float*   tag_corners;   /* T x 4 x 3 object-frame corners, the reference's template order */
    int32_t        n_samples;     /* 1 <= M <= 4,194,304 */
    int32_t        facing;        /* +1 or -1: the sign of the tag normal (agt_tracker_visibility) */
    const float*   model_xyz;     /* M x 3 object-frame samples */
    const int32_t* sample_tag;    /* M: the tag a sample lies on */
    double         max_view_deg;  /* (0, 90] */
} agt_model_problem;

typedef struct agt_dense_model agt_dense_model;

int agt_model_version(void);

/* Checks the problem (all refusals before any device work) and uploads it once.  stream: a hipStream_t (NULL = the default stream).
 * The problem's arrays are not retained. */
int agt_dense_model_create(const agt_model_problem* problem, void* stream, agt_dense_model** handle_out);
int agt_dense_model_destroy(agt_dense_model* handle);

/* Opens a pass: clip_sigma = 0 is the plain pass; clip_sigma > 0 is a clipped pass whose reference is the previous pass, which must
 * have had at least one accumulate call.  The accumulators and the pass's frame counter go to zero. */
int agt_dense_model_begin_pass(agt_dense_model* handle, double clip_sigma, double sigma_floor);

/* `count` frames (device memory, u8, frame k at d_frames + k * frame_stride, rows `pitch` bytes apart, pitch >= width) with their
 * poses (host, count x 6) and use bytes (host, count; NULL = all used).  frame_obs_out: host, count, or NULL. */
int agt_dense_model_accumulate(agt_dense_model* handle, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int count,
                               const double* poses, const uint8_t* use, int32_t* frame_obs_out);

/* The current pass's raw sums; each array is M long and may be NULL. */
int agt_dense_model_read(agt_dense_model* handle, int32_t* n, double* S, double* S2, int32_t* rejected);

#ifdef __cplusplus
}
#endif
#endif
