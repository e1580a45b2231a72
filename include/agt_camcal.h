/*
 * agt_camcal.h -- C ABI of libagt_camcal.so: offline calibration of the camera itself (the CameraParams.npz every other tool takes as
 * given) from views of a rigid target, by Levenberg-Marquardt on the MI355X (gfx950).
 *
 * The problem (fixed; tests/camera_calib_numpy.py states it independently):
 *   views      V views (1..65536) of one rigid target; view v has n_v points (4..4096), each a target coordinate X (3 doubles) and an
 *              observed pixel (2 doubles); view_start (V + 1 offsets into the point arrays) carries the variable counts.  Views and
 *              points are used in the caller's order.
 *   unknowns   p_v = (rvec, tvec) target -> camera for every view, and the shared camera vector
 *              c[16] = fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 s1 s2 s3 s4
 *   free mask  bit i set: c[i] is estimated.  A fixed entry keeps the bits it was given and gets a step of exactly 0.  The tilt
 *              (tau_x, tau_y) of the 14-coefficient model is not estimated and not modelled: ndist = 14 is AGT_CAMCAL_ERR_CAMERA.
 *   residual   project(c, R(p_v.r), p_v.t, X) - observed   (the projection of agt_project_points), two rows per point
 *   cost       1/2 sum r^2 -- the cost cv2.calibrateCamera minimises
 * The minimiser is this project's Levenberg-Marquardt (include/agt_calib.h): Marquardt scaling with the diagonal of each block, the
 * same options, report and stop reasons.  It is NOT a restatement of OpenCV's CvLevMarq: the two reach the same minimum of the same
 * cost by different paths, and parity with cv2.calibrateCamera's iterates or iteration counts is not pinned anywhere.
 *
 * Per point J = [J_c (2 x 16) | J_v (2 x 6)]; per view A_v = sum J_c^T J_c, B_v = sum J_c^T J_v, U_v = sum J_v^T J_v, g_c,v, g_v;
 * A = sum_v A_v.  The view poses are eliminated:
 *     S = A + lambda diag A - sum_v B_v (U_v + lambda diag U_v)^-1 B_v^T                    (<= 16 unknowns, solved on the host)
 *     d_v = -(U_v + lambda diag U_v)^-1 (g_v + B_v^T d_c)
 * Everything on the device is FP64 and every sum runs in a fixed order (no floating-point atomics): two solves of one problem are
 * bitwise equal.
 *
 * Conventions (those of agt_calib.h): every function returns 0 or a negative AGT_CAMCAL_ERR_*; nothing throws.  The calls are
 * synchronous and take HOST arrays; poses are 6 doubles, rvec then tvec.  Every argument check happens before any device work.
 * A handle is not re-entrant.
 */
#ifndef AGT_CAMCAL_H
#define AGT_CAMCAL_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define AGT_CAMCAL_VERSION 100

#define AGT_CAMCAL_OK               0
#define AGT_CAMCAL_ERR_ARG        (-1)   /* NULL pointer, V outside 1..65536, a view outside 4..4096 points, offsets that do not start at 0 or ascend, bits above 15 in the mask */
#define AGT_CAMCAL_ERR_ALLOC      (-2)
#define AGT_CAMCAL_ERR_CAMERA     (-3)   /* ndist not in {0,4,5,8,12} (14, the tilted model, included), or a free coefficient beyond ndist */
#define AGT_CAMCAL_ERR_HIP        (-5)   /* a HIP runtime call failed */
#define AGT_CAMCAL_ERR_TOO_FEW   (-10)   /* fewer residuals than unknowns: 2 sum n_v < 6 V + popcount(free) */
#define AGT_CAMCAL_ERR_SINGULAR  (-11)   /* agt_camcal_step: the damped system is not positive definite */
#define AGT_CAMCAL_ERR_DEGENERATE (-12)  /* raised by the Python start (camera_calib.py), never by this library: no focal length from the views */

#define AGT_CAMCAL_MAX_VIEWS        65536
#define AGT_CAMCAL_MIN_VIEW_POINTS  4
#define AGT_CAMCAL_MAX_VIEW_POINTS  4096
#define AGT_CAMCAL_NCAM             16

/* why agt_camcal_solve stopped (the values of AGT_CALIB_STOP_*) */
#define AGT_CAMCAL_STOP_CONVERGED  1   /* an accepted step lowered the cost by less than ftol (relative) */
#define AGT_CAMCAL_STOP_MAX_ITERS  2
#define AGT_CAMCAL_STOP_LAMBDA     3   /* no step was accepted up to the largest damping */

typedef struct agt_camcal_problem {
    int32_t        n_views;        /* V */
    int32_t        ndist;          /* the distortion model: 0, 4, 5, 8 or 12 coefficients may be free; the others stay as given */
    uint32_t       free_mask;      /* bit i: c[i] is estimated */
    int32_t        reserved0;
    const int32_t* view_start;     /* V + 1: the points of view v are view_start[v] .. view_start[v + 1]; view_start[0] = 0 */
    const double*  object_points;  /* view_start[V] x 3, target coordinates */
    const double*  image_points;   /* view_start[V] x 2, observed pixels */
} agt_camcal_problem;

/* the layouts of agt_calib_options / agt_calib_report */
typedef struct agt_camcal_options {
    int32_t max_iters;            /* LM iterations (damped solves), accepted or not */
    int32_t reserved0;
    double  ftol;                 /* stop when an accepted step lowers the cost by less than ftol * cost */
    double  lambda0;              /* initial damping */
    double  lambda_up;            /* factor after a rejected step (> 1) */
    double  lambda_down;          /* factor after an accepted step (< 1) */
    double  lambda_max;           /* give up beyond */
} agt_camcal_options;

typedef struct agt_camcal_report {
    int32_t iterations;
    int32_t accepted;
    int32_t stop_reason;          /* AGT_CAMCAL_STOP_* */
    int32_t n_residuals;          /* 2 per point */
    double  initial_cost;
    double  final_cost;
    double  final_rms_px;         /* sqrt(2 cost / n_residuals) */
    double  final_lambda;
} agt_camcal_report;

typedef struct agt_camcal agt_camcal;

int agt_camcal_version(void);

/* Checks the problem (argument errors, the view sizes, the counting rule, the camera model -- all before any device work) and
 * uploads it once.  stream: a hipStream_t (NULL = the default stream).  The problem's arrays are not retained. */
int agt_camcal_create(const agt_camcal_problem* problem, void* stream, agt_camcal** handle_out);
int agt_camcal_destroy(agt_camcal* handle);

/* Residuals (view_start[V] x 2, projected - observed, in the caller's point order; may be NULL) and the cost at camera[16], view_poses[V x 6]. */
int agt_camcal_eval(agt_camcal* handle, const double* camera, const double* view_poses, double* residuals_out, double* cost_out);

/* One damped step at the given camera and poses through the Schur path; applies nothing.  d_camera_out: 16 (exactly 0 for a fixed
 * entry), d_views_out: V x 6. */
int agt_camcal_step(agt_camcal* handle, double lambda, const double* camera, const double* view_poses, double* d_camera_out, double* d_views_out);

/* Levenberg-Marquardt from the given camera and poses (both in/out).  options: NULL = agt_camcal_default_options. */
int agt_camcal_default_options(agt_camcal_options* options);
int agt_camcal_solve(agt_camcal* handle, const agt_camcal_options* options, double* camera, double* view_poses, agt_camcal_report* report);

#ifdef __cplusplus
}
#endif
#endif
