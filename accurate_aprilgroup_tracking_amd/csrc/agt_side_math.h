// agt_side_math.h -- host code shared by the side libraries (libagt_calib.so, libagt_camcal.so, libagt_model.so) and agt_api.hip:
// the codes they have in common, the dense Cholesky of the reduced systems, the tilted-sensor matrices, the camera fill and the
// Levenberg-Marquardt loop.  Plain C++: no HIP header, so tests/side_math_check.cpp drives it on a CPU under the sanitizers.
// Floating-point contraction: none.  Include it in front of a file's own `#pragma clang fp contract`, where the command line's
// -ffp-contract=off holds.
#pragma once
#include <math.h>
#include <string.h>
#include <vector>

namespace agt_side {

// every side library's header gives these the same values under its own prefix (a static_assert in each .hip file holds it to that)
enum { OK = 0, ERR_ARG = -1, ERR_ALLOC = -2, ERR_HIP = -5 };
enum { STOP_CONVERGED = 1, STOP_MAX_ITERS = 2, STOP_LAMBDA = 3 };

// in-place Cholesky A = L L^T (lower triangle of the row-major n x n A), then A x = b in b; false on a non-positive pivot
inline bool cholesky_solve(std::vector<double>& A, std::vector<double>& b, int n)
{
    for (int j = 0; j < n; j++) {
        double d = A[(size_t)j * n + j];
        for (int k = 0; k < j; k++) d -= A[(size_t)j * n + k] * A[(size_t)j * n + k];
        if (!(d > 0.0) || !isfinite(d)) return false;
        d = sqrt(d);
        A[(size_t)j * n + j] = d;
        for (int i = j + 1; i < n; i++) {
            double v = A[(size_t)i * n + j];
            for (int k = 0; k < j; k++) v -= A[(size_t)i * n + k] * A[(size_t)j * n + k];
            A[(size_t)i * n + j] = v / d;
        }
    }
    for (int i = 0; i < n; i++) {
        double v = b[i];
        for (int k = 0; k < i; k++) v -= A[(size_t)i * n + k] * b[k];
        b[i] = v / A[(size_t)i * n + i];
    }
    for (int i = n - 1; i >= 0; i--) {
        double v = b[i];
        for (int k = i + 1; k < n; k++) v -= A[(size_t)k * n + i] * b[k];
        b[i] = v / A[(size_t)i * n + i];
    }
    return true;
}

// matTilt (m[0..8]) | invMatTilt (m[9..17]) of the 14-coefficient model (OpenCV's detail::computeTiltProjectionMatrix<double>,
// distortion_model.hpp; Matx products accumulate s = 0; s += a * b)
inline void tilt_matrices(double tau_x, double tau_y, double* m)
{
    const double cX = cos(tau_x), sX = sin(tau_x), cY = cos(tau_y), sY = sin(tau_y);
    const double rotX[9] = { 1, 0, 0, 0, cX, sX, 0, -sX, cX }, rotY[9] = { cY, 0, -sY, 0, 1, 0, sY, 0, cY };
    auto mul = [](const double* A, const double* B, double* C) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) { double a = 0; for (int q = 0; q < 3; q++) a += A[i * 3 + q] * B[q * 3 + j]; C[i * 3 + j] = a; }
    };
    double rotXY[9];
    mul(rotY, rotX, rotXY);
    const double projZ[9] = { rotXY[8], 0, -rotXY[2], 0, rotXY[8], -rotXY[5], 0, 0, 1 };
    mul(projZ, rotXY, m);
    const double inv = 1. / rotXY[8];
    const double invProjZ[9] = { inv, 0, inv * rotXY[2], 0, inv, inv * rotXY[5], 0, 0, 1 };
    const double rt[9] = { rotXY[0], rotXY[3], rotXY[6], rotXY[1], rotXY[4], rotXY[7], rotXY[2], rotXY[5], rotXY[8] };
    mul(rt, invProjZ, m + 9);
}

// A problem's camera (K 3 x 3, nd checked coefficients) into a kernel argument: intrinsics and the 12 polynomial coefficients by value,
// the tilt pointer null.  True when the model is tilted: then m holds the matrices, and the caller uploads them and sets cam.tilt.
template <class Camera>
bool fill_camera(const double* K, const double* dist, int nd, Camera& cam, double m[18])
{
    cam.fx = K[0]; cam.fy = K[4]; cam.cx = K[2]; cam.cy = K[5];
    for (int i = 0; i < 12; i++) cam.k[i] = i < nd ? dist[i] : 0.0;
    cam.tilt = nullptr;
    if (!(nd == 14 && (dist[12] != 0.0 || dist[13] != 0.0))) return false;
    tilt_matrices(dist[12], dist[13], m);
    return true;
}

// ---- Levenberg-Marquardt: one loop for every library whose options and report have the layout of agt_calib_options / agt_calib_report

template <class Options>
void lm_default_options(Options* o)
{
    memset(o, 0, sizeof(*o));
    o->max_iters = 50; o->ftol = 1e-14; o->lambda0 = 1e-3; o->lambda_up = 10.0; o->lambda_down = 0.1; o->lambda_max = 1e12;
}

// the options of a solve: the defaults, or the caller's; false when one of them is refused
template <class Options>
bool lm_options(const Options* given, Options& o)
{
    lm_default_options(&o);
    if (given) o = *given;
    return !(o.max_iters < 0 || !(o.ftol >= 0.0) || !(o.lambda0 >= 0.0) || !(o.lambda_up > 1.0) || !(o.lambda_down > 0.0) || !(o.lambda_down <= 1.0) ||
             !(o.lambda_max > 0.0));
}

// The loop from a point of cost cost0.
//   step(lambda, cost_trial) -> return code   the damped step at the current point; when it is solved, forms the trial point, evaluates
//                                             it and stores its cost; leaves cost_trial (INFINITY) alone when it is not: a rejection
//   commit()                                  the trial point becomes the current one
// A non-zero code of step ends the solve with that code and without a report.  The report is filled whole (n_residuals as given).
template <class Options, class Report, class Step, class Commit>
int lm_solve(const Options& o, double cost0, int n_residuals, Step step, Commit commit, Report* report)
{
    double cost = cost0, lambda = o.lambda0;
    int iters = 0, accepted = 0, stop = STOP_MAX_ITERS;
    while (iters < o.max_iters) {
        if (cost == 0.0) { stop = STOP_CONVERGED; break; }
        iters++;
        double cost_trial = INFINITY;
        const int rc = step(lambda, cost_trial);
        if (rc) return rc;
        if (cost_trial < cost) {                        // (NaN fails)
            const double gain = cost - cost_trial;
            commit(); accepted++;
            const bool done = gain <= o.ftol * cost;
            cost = cost_trial;
            lambda *= o.lambda_down;
            if (done) { stop = STOP_CONVERGED; break; }
        } else {
            lambda = lambda > 0.0 ? lambda * o.lambda_up : 1e-6;
            if (lambda > o.lambda_max) { stop = STOP_LAMBDA; break; }
        }
    }
    memset(report, 0, sizeof(*report));
    report->iterations = iters; report->accepted = accepted; report->stop_reason = stop; report->n_residuals = n_residuals;
    report->initial_cost = cost0; report->final_cost = cost;
    report->final_rms_px = n_residuals ? sqrt(2.0 * cost / (double)n_residuals) : 0.0;
    report->final_lambda = lambda;
    return OK;
}

}  // namespace agt_side
