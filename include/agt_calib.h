/*
 * agt_calib.h -- C ABI of libagt_calib.so: offline calibration of an AprilGroup (the april_group.json the tracker reads)
 * from a detection recording, by bundle adjustment on the MI355X (gfx950).
 *
 * The problem (fixed; tests/group_ba_numpy.py states it independently):
 *   unknowns   p_f = (rvec, tvec) body -> camera for every frame f < F, q_t = (rvec, tvec) tag -> body for every tag t < T;
 *              one tag, the anchor, keeps the extrinsics it is given
 *   corner k of tag t in the tag frame, r = size_t / 2:  (-r,-r,0), (-r,r,0), (r,r,0), (r,-r,0)   (the reference's template order)
 *   X = R(q_t.r) c_k + q_t.t,   pixel = project(camera, R(p_f.r), p_f.t, X)   (the projection of agt_project_points, tilt included)
 *   residual = projected - observed, two rows per corner;   cost = 1/2 sum r^2
 * Everything on the device is FP64.  The solver is Levenberg-Marquardt with Marquardt scaling (D = the diagonal of each block) and
 * the frame poses eliminated (Schur complement); every sum runs in a fixed order, so two solves of one problem are bitwise equal.
 *
 * Conventions: every function returns 0 or a negative AGT_CALIB_ERR_*; nothing throws.  The calls are synchronous and take HOST
 * arrays (the style of agt_solve_pnp_host); poses are 6 doubles, rvec then tvec.  A handle is not re-entrant.
 * This is an offline tool, separate from the per-frame library (include/agt_hip.h), which it neither needs nor changes.
 */
#ifndef AGT_CALIB_H
#define AGT_CALIB_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_CALIB_VERSION 100

#define AGT_CALIB_OK                    0
#define AGT_CALIB_ERR_ARG             (-1)   /* NULL pointer, T outside 1..64, F outside 1..65536, an index out of range, a tag seen twice in a frame */
#define AGT_CALIB_ERR_ALLOC           (-2)
#define AGT_CALIB_ERR_CAMERA          (-3)   /* unknown camera model: distortion count not in {0,4,5,8,12,14} */
#define AGT_CALIB_ERR_HIP             (-5)   /* a HIP runtime call failed */
#define AGT_CALIB_ERR_DISCONNECTED    (-9)   /* a tag has no path to the anchor through frames that saw two tags together */
#define AGT_CALIB_ERR_TOO_FEW_FRAMES (-10)   /* fewer than two frames with a usable observation */
#define AGT_CALIB_ERR_SINGULAR       (-11)   /* agt_group_calib_step: the damped system is not positive definite */

#define AGT_CALIB_MAX_TAGS   64
#define AGT_CALIB_MAX_FRAMES 65536

/* why agt_group_calib_solve stopped */
#define AGT_CALIB_STOP_CONVERGED  1   /* an accepted step lowered the cost by less than ftol (relative) */
#define AGT_CALIB_STOP_MAX_ITERS  2
#define AGT_CALIB_STOP_LAMBDA     3   /* no step was accepted up to the largest damping */

typedef struct agt_calib_problem {
    const double*  K;             /* 3 x 3 row-major camera matrix */
    const double*  dist;          /* ndist distortion coefficients (k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4 tau_x tau_y), NULL when ndist = 0 */
    int32_t        ndist;         /* 0, 4, 5, 8, 12 or 14 */
    int32_t        n_tags;        /* T <= 64 */
    const double*  tag_sizes;     /* T edge lengths */
    int32_t        anchor;        /* the tag held fixed */
    int32_t        n_frames;      /* F <= 65536 */
    int32_t        n_obs;         /* rows of the observation table, any order (the library sorts by frame, stably) */
    int32_t        reserved0;
    const int32_t* obs_frame;     /* n_obs */
    const int32_t* obs_tag;       /* n_obs */
    const double*  obs_corners;   /* n_obs x 8: (x, y) of corners 0..3 in the template order */
} agt_calib_problem;

typedef struct agt_calib_options {
    int32_t max_iters;            /* LM iterations (damped solves), accepted or not */
    int32_t reserved0;
    double  ftol;                 /* stop when an accepted step lowers the cost by less than ftol * cost */
    double  lambda0;              /* initial damping */
    double  lambda_up;            /* factor after a rejected step (> 1) */
    double  lambda_down;          /* factor after an accepted step (< 1) */
    double  lambda_max;           /* give up beyond */
} agt_calib_options;

typedef struct agt_calib_report {
    int32_t iterations;
    int32_t accepted;
    int32_t stop_reason;          /* AGT_CALIB_STOP_* */
    int32_t n_residuals;          /* 8 per observation */
    double  initial_cost;
    double  final_cost;
    double  final_rms_px;         /* sqrt(2 cost / n_residuals) */
    double  final_lambda;
} agt_calib_report;

typedef struct agt_group_calib agt_group_calib;

int agt_calib_version(void);

/* Checks the problem (argument errors, camera model, usable frames, co-visibility graph -- all before any device work), sorts the
 * table by frame and uploads it once.  stream: a hipStream_t (NULL = the default stream).  The problem's arrays are not retained. */
int agt_group_calib_create(const agt_calib_problem* problem, void* stream, agt_group_calib** handle_out);
int agt_group_calib_destroy(agt_group_calib* handle);

/* Residuals (n_obs x 8, projected - observed, in the CALLER's observation order; may be NULL) and the cost at the given poses. */
int agt_group_calib_eval(agt_group_calib* handle, const double* tag_poses, const double* frame_poses, double* residuals_out, double* cost_out);

/* One damped step at the given poses through the Schur path; applies nothing.  d_tags_out: T x 6 (zeros for the anchor),
 * d_frames_out: F x 6 (zeros for a frame without observations). */
int agt_group_calib_step(agt_group_calib* handle, double lambda, const double* tag_poses, const double* frame_poses,
                         double* d_tags_out, double* d_frames_out);

/* Levenberg-Marquardt from the given poses (in/out).  options: NULL = agt_group_calib_default_options. */
int agt_group_calib_default_options(agt_calib_options* options);
int agt_group_calib_solve(agt_group_calib* handle, const agt_calib_options* options, double* tag_poses, double* frame_poses,
                          agt_calib_report* report);

#ifdef __cplusplus
}
#endif
#endif
