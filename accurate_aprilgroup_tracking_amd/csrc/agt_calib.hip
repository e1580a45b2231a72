// agt_calib.hip -- libagt_calib.so (include/agt_calib.h): bundle adjustment of an AprilGroup from a detection recording.
//
// Levenberg-Marquardt over tag poses q_t and frame poses p_f with the frame poses eliminated.  With J = [J_f | J_t] per observation
// (one tag seen in one frame: 4 corners, 8 residual rows) the normal equations are
//     [ U   W ] [d_f]     [g_f]        U_f = sum J_f^T J_f (6x6 per frame),  V_t = sum J_t^T J_t (6x6 per tag),
//     [ W^T V ] [d_t] = - [g_t]        W_{f,t} = J_f^T J_t (6x6 per observation)
// and, with A_f = U_f + lambda diag(U_f), Y_{f,t} = A_f^-1 W_{f,t}, x_f = A_f^-1 g_f:
//     S d_t = -(g_t - sum_f W_{f,t}^T x_f),   S_{t1,t2} = [t1 == t2] (V_t + lambda diag V_t) - sum_f W_{f,t1}^T Y_{f,t2}
//     d_f = -x_f - sum_t Y_{f,t} d_t
// Kernels (all FP64, every sum in a fixed order -- no floating-point atomics, so a solve is reproducible to the bit):
//     calib_accumulate_kernel   one thread per observation: residuals, both 2x6 Jacobian blocks, its terms of U, V, g and its W
//     calib_eliminate_kernel    one thread per observation: A_f (the frame's terms summed in table order), Y; the frame's first: x_f
//     calib_reduce_kernel       one workgroup per block (t1 <= t2) that some frame saw together: frames in order, 16 fixed segments
//     calib_backsub_kernel      one thread per frame: d_f and the trial pose
//     calib_cost_kernel         one workgroup: per frame, then over frames (strided, then a fixed tree)
// The reduced system (6 (T - 1) <= 378 unknowns) is solved on the host by a plain Cholesky; the LM loop is host code.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "agt_device.h"
#include "agt_side_buffers.h"
#include "agt_side_device.h"
#include "../../include/agt_calib.h"

#pragma clang fp contract(fast)

static_assert(AGT_CALIB_OK == agt_side::OK && AGT_CALIB_ERR_ARG == agt_side::ERR_ARG && AGT_CALIB_ERR_ALLOC == agt_side::ERR_ALLOC &&
              AGT_CALIB_ERR_HIP == agt_side::ERR_HIP && AGT_CALIB_STOP_CONVERGED == agt_side::STOP_CONVERGED &&
              AGT_CALIB_STOP_MAX_ITERS == agt_side::STOP_MAX_ITERS && AGT_CALIB_STOP_LAMBDA == agt_side::STOP_LAMBDA,
              "the shared host code returns this library's codes");

namespace {

#define CALIB_SEGMENTS 16          // calib_reduce_kernel: waves per workgroup = frame segments of the fixed summation tree

struct CalibDev {                  // the uploaded problem (kernel argument, by value)
    AgtCamera cam;
    int n, F, T, rsv_;
    const int* obs_tag;            // n, sorted by frame
    const int* obs_frame;          // n
    const int* fstart;             // F + 1: observations of frame f are fstart[f] .. fstart[f + 1]
    const int* obs_of;             // T x F: the observation of tag t in frame f, or -1
    const double* obs_c;           // n x 8
    const double* sizes;           // T
};

struct CalibSet {                  // what calib_accumulate_kernel writes for one set of poses
    double* U;                     // n x 36  J_f^T J_f of the observation
    double* W;                     // n x 36  J_f^T J_t   [frame parameter][tag parameter]
    double* V;                     // n x 36  J_t^T J_t
    double* gf;                    // n x 6   J_f^T r
    double* gt;                    // n x 6   J_t^T r
    double* res;                   // n x 8
    double* cost;                  // n       1/2 sum r^2
};

__global__ __launch_bounds__(64) void calib_accumulate_kernel(CalibDev P, const double* __restrict__ tag_pose, const double* __restrict__ frame_pose, CalibSet S)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= P.n) return;
    const int t = P.obs_tag[o], f = P.obs_frame[o];
    double pf[6], qt[6];
#pragma unroll
    for (int i = 0; i < 6; i++) { pf[i] = frame_pose[f * 6 + i]; qt[i] = tag_pose[t * 6 + i]; }
    double Rf[9], Gf[9], Rt[9], Gt[9];
    agt_rodrigues<true>(pf, Rf, Gf);
    agt_rodrigues<true>(qt, Rt, Gt);
    const double tf[3] = { pf[3], pf[4], pf[5] };
    const double r = 0.5 * P.sizes[t];
    double U[21], V[21], W[36], gf[6], gt[6], cost = 0.0;
#pragma unroll
    for (int i = 0; i < 21; i++) { U[i] = 0.0; V[i] = 0.0; }
#pragma unroll
    for (int i = 0; i < 36; i++) W[i] = 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) { gf[i] = 0.0; gt[i] = 0.0; }
#pragma unroll 1
    for (int k = 0; k < 4; k++) {
        const double cx = k >= 2 ? r : -r, cy = (k == 1 || k == 2) ? r : -r;            // the reference's corner template
        const double c0 = Rt[0] * cx + Rt[1] * cy, c1 = Rt[3] * cx + Rt[4] * cy, c2 = Rt[6] * cx + Rt[7] * cy;      // R_t c
        double u, v, jr[6], jt[6];
        agt_project<true, true>(P.cam, Rf, Gf, tf, c0 + qt[3], c1 + qt[4], c2 + qt[5], u, v, jr, jt);
        const double ru = u - P.obs_c[o * 8 + 2 * k], rv = v - P.obs_c[o * 8 + 2 * k + 1];
        S.res[o * 8 + 2 * k] = ru; S.res[o * 8 + 2 * k + 1] = rv;
        cost += ru * ru + rv * rv;
        // rows (u, v) of both blocks; parameters: rvec, tvec
        double Jf[2][6], Jt[2][6], M[2][3];
#pragma unroll
        for (int a = 0; a < 2; a++) {
#pragma unroll
            for (int j = 0; j < 3; j++) {
                Jf[a][j] = jr[a * 3 + j]; Jf[a][3 + j] = jt[a * 3 + j];
                M[a][j] = jt[a * 3] * Rf[j] + jt[a * 3 + 1] * Rf[3 + j] + jt[a * 3 + 2] * Rf[6 + j];       // d pixel / d X = jt R_f
            }
        }
#pragma unroll
        for (int j = 0; j < 3; j++) {
            const double gx = Gt[j], gy = Gt[3 + j], gz = Gt[6 + j];                     // d X / d q.r_j = G_j x (R_t c)
            const double d0 = gy * c2 - gz * c1, d1 = gz * c0 - gx * c2, d2 = gx * c1 - gy * c0;
#pragma unroll
            for (int a = 0; a < 2; a++) { Jt[a][j] = M[a][0] * d0 + M[a][1] * d1 + M[a][2] * d2; Jt[a][3 + j] = M[a][j]; }
        }
        int q = 0;
#pragma unroll
        for (int i = 0; i < 6; i++) {
            gf[i] += Jf[0][i] * ru + Jf[1][i] * rv;
            gt[i] += Jt[0][i] * ru + Jt[1][i] * rv;
#pragma unroll
            for (int j = 0; j < 6; j++) {
                W[i * 6 + j] += Jf[0][i] * Jt[0][j] + Jf[1][i] * Jt[1][j];
                if (j >= i) {
                    U[q] += Jf[0][i] * Jf[0][j] + Jf[1][i] * Jf[1][j];
                    V[q] += Jt[0][i] * Jt[0][j] + Jt[1][i] * Jt[1][j];
                    q++;
                }
            }
        }
    }
    S.cost[o] = 0.5 * cost;
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; i++) {
        S.gf[o * 6 + i] = gf[i]; S.gt[o * 6 + i] = gt[i];
#pragma unroll
        for (int j = 0; j < 6; j++) {
            S.W[(size_t)o * 36 + i * 6 + j] = W[i * 6 + j];
            if (j >= i) {
                S.U[(size_t)o * 36 + i * 6 + j] = U[q]; S.U[(size_t)o * 36 + j * 6 + i] = U[q];
                S.V[(size_t)o * 36 + i * 6 + j] = V[q]; S.V[(size_t)o * 36 + j * 6 + i] = V[q];
                q++;
            }
        }
    }
}

__global__ __launch_bounds__(64) void calib_eliminate_kernel(CalibDev P, CalibSet S, double lambda, double* __restrict__ Y, double* __restrict__ xf, int* __restrict__ fail)
{
    const int o = blockIdx.x * 64 + threadIdx.x;
    if (o >= P.n) return;
    const int f = P.obs_frame[o], o0 = P.fstart[f], o1 = P.fstart[f + 1];
    double A[36];
#pragma unroll
    for (int e = 0; e < 36; e++) A[e] = 0.0;
    for (int p = o0; p < o1; p++) {
#pragma unroll
        for (int e = 0; e < 36; e++) A[e] += S.U[(size_t)p * 36 + e];
    }
#pragma unroll
    for (int i = 0; i < 6; i++) A[i * 7] += lambda * A[i * 7];
    AgtLdl6 F;
    const bool ok = agt_ldl6_factor(A, F);
#pragma unroll 1
    for (int j = 0; j < 6; j++) {
        double b[6], x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) b[k] = S.W[(size_t)o * 36 + k * 6 + j];
        agt_ldl6_subst(F, b, x);
#pragma unroll
        for (int k = 0; k < 6; k++) Y[(size_t)o * 36 + k * 6 + j] = x[k];
    }
    if (o == o0) {
        double b[6], x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) b[k] = 0.0;
        for (int p = o0; p < o1; p++) {
#pragma unroll
            for (int k = 0; k < 6; k++) b[k] += S.gf[p * 6 + k];
        }
        agt_ldl6_subst(F, b, x);
#pragma unroll
        for (int k = 0; k < 6; k++) xf[f * 6 + k] = x[k];
    }
    if (!ok) *fail = 1;
}

__global__ __launch_bounds__(64 * CALIB_SEGMENTS) void calib_reduce_kernel(CalibDev P, CalibSet S, const int* __restrict__ pairs, double lambda,
                                                                          const double* __restrict__ Y, const double* __restrict__ xf,
                                                                          double* __restrict__ S_out, double* __restrict__ rhs_out)
{
    __shared__ double part[CALIB_SEGMENTS][2][48];
    const int t1 = pairs[blockIdx.x * 2], t2 = pairs[blockIdx.x * 2 + 1];
    const int e = threadIdx.x & 63, c = threadIdx.x >> 6;
    const int per = (P.F + CALIB_SEGMENTS - 1) / CALIB_SEGMENTS;
    const int f0 = c * per, f1 = min(P.F, f0 + per);
    const bool diag = t1 == t2;
    double a = 0.0, b = 0.0;           // a: V (or g_t), b: W^T Y (or W^T x)
    if (e < 36) {
        const int i = e / 6, j = e % 6;
        for (int f = f0; f < f1; f++) {
            const int p1 = P.obs_of[t1 * P.F + f];
            if (p1 < 0) continue;
            const int p2 = diag ? p1 : P.obs_of[t2 * P.F + f];
            if (p2 < 0) continue;
            if (diag) a += S.V[(size_t)p1 * 36 + e];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) s += S.W[(size_t)p1 * 36 + k * 6 + i] * Y[(size_t)p2 * 36 + k * 6 + j];
            b += s;
        }
    } else if (e < 42 && diag) {
        const int i = e - 36;
        for (int f = f0; f < f1; f++) {
            const int p1 = P.obs_of[t1 * P.F + f];
            if (p1 < 0) continue;
            a += S.gt[p1 * 6 + i];
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 6; k++) s += S.W[(size_t)p1 * 36 + k * 6 + i] * xf[f * 6 + k];
            b += s;
        }
    }
    if (e < 48) { part[c][0][e] = a; part[c][1][e] = b; }
    __syncthreads();
    if (c == 0 && e < 42) {
        double sa = 0.0, sb = 0.0;
        for (int s = 0; s < CALIB_SEGMENTS; s++) { sa += part[s][0][e]; sb += part[s][1][e]; }
        if (e < 36) {
            if (e / 6 == e % 6) sa += lambda * sa;
            S_out[blockIdx.x * 36 + e] = sa - sb;
        } else if (diag) {
            rhs_out[t1 * 6 + (e - 36)] = sa - sb;
        }
    }
}

__global__ __launch_bounds__(64) void calib_backsub_kernel(CalibDev P, const double* __restrict__ Y, const double* __restrict__ xf, const double* __restrict__ d_tag,
                                                           const double* __restrict__ frame_pose, double* __restrict__ d_frame, double* __restrict__ frame_trial)
{
    const int f = blockIdx.x * 64 + threadIdx.x;
    if (f >= P.F) return;
    const int o0 = P.fstart[f], o1 = P.fstart[f + 1];
    double d[6];
#pragma unroll
    for (int k = 0; k < 6; k++) d[k] = o1 > o0 ? -xf[f * 6 + k] : 0.0;
    for (int p = o0; p < o1; p++) {
        const int t = P.obs_tag[p];
#pragma unroll
        for (int k = 0; k < 6; k++) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < 6; j++) s += Y[(size_t)p * 36 + k * 6 + j] * d_tag[t * 6 + j];
            d[k] -= s;
        }
    }
#pragma unroll
    for (int k = 0; k < 6; k++) { d_frame[f * 6 + k] = d[k]; frame_trial[f * 6 + k] = frame_pose[f * 6 + k] + d[k]; }
}

__global__ __launch_bounds__(1024) void calib_cost_kernel(CalibDev P, const double* __restrict__ cost_o, double* __restrict__ cost_out)
{
    __shared__ double part[1024];
    double acc = 0.0;
    for (int f = threadIdx.x; f < P.F; f += 1024) {
        double cf = 0.0;
        for (int p = P.fstart[f]; p < P.fstart[f + 1]; p++) cf += cost_o[p];
        acc += cf;
    }
    agt_block_sum_1024(acc, part);
    if (threadIdx.x == 0) cost_out[0] = part[0];
}

}  // namespace

struct agt_group_calib {
    AgtSideBuffers dev;
    CalibDev P;
    int T, F, n, anchor, n_pairs, n_used_frames;
    std::vector<int> perm;             // sorted row -> the caller's row
    std::vector<int> pairs;            // (t1, t2), t1 <= t2, neither the anchor
    CalibSet set[2];
    double *d_tag[2], *d_frame[2];
    double *d_Y, *d_xf, *d_S, *d_rhs, *d_dtag, *d_dframe, *d_cost, *d_tilt;
    int *d_pairs, *d_fail;
    int cur;
};

namespace {

inline int blocks64(int n) { return (n + 63) / 64; }

// residuals, Jacobian products and the cost of set s at (d_tag[s], d_frame[s])
int accumulate(agt_group_calib* h, int s, double* cost)
{
    if (h->n) calib_accumulate_kernel<<<blocks64(h->n), 64, 0, h->dev.stream>>>(h->P, h->d_tag[s], h->d_frame[s], h->set[s]);
    calib_cost_kernel<<<1, 1024, 0, h->dev.stream>>>(h->P, h->set[s].cost, h->d_cost);
    HC(hipGetLastError());
    return h->dev.download(cost, h->d_cost, sizeof(double));
}

// the damped step at set s: d_tag (host, T x 6) and, on the device, d_dframe and the trial frame poses in d_frame[1 - s]
int damped_step(agt_group_calib* h, int s, double lambda, std::vector<double>& d_tag, bool* solved)
{
    const int T = h->T, nr = 6 * (T - 1);
    *solved = false;
    HC(hipMemsetAsync(h->d_fail, 0, sizeof(int), h->dev.stream));
    if (h->n) calib_eliminate_kernel<<<blocks64(h->n), 64, 0, h->dev.stream>>>(h->P, h->set[s], lambda, h->d_Y, h->d_xf, h->d_fail);
    if (h->n_pairs)
        calib_reduce_kernel<<<h->n_pairs, 64 * CALIB_SEGMENTS, 0, h->dev.stream>>>(h->P, h->set[s], h->d_pairs, lambda, h->d_Y, h->d_xf, h->d_S, h->d_rhs);
    HC(hipGetLastError());
    std::vector<double> blk((size_t)h->n_pairs * 36), rhs((size_t)T * 6, 0.0);
    int fail = 0;
    HC(hipMemcpyAsync(blk.data(), h->d_S, blk.size() * sizeof(double), hipMemcpyDeviceToHost, h->dev.stream));
    HC(hipMemcpyAsync(rhs.data(), h->d_rhs, rhs.size() * sizeof(double), hipMemcpyDeviceToHost, h->dev.stream));
    HC(hipMemcpyAsync(&fail, h->d_fail, sizeof(int), hipMemcpyDeviceToHost, h->dev.stream));
    HC(hipStreamSynchronize(h->dev.stream));
    if (fail) return AGT_CALIB_OK;
    std::vector<double> A((size_t)nr * nr, 0.0), b(nr, 0.0);
    auto ri = [&](int t) { return t < h->anchor ? t : t - 1; };
    for (int p = 0; p < h->n_pairs; p++) {
        const int r1 = ri(h->pairs[2 * p]) * 6, r2 = ri(h->pairs[2 * p + 1]) * 6;
        for (int i = 0; i < 6; i++)
            for (int j = 0; j < 6; j++) {
                const double v = blk[(size_t)p * 36 + i * 6 + j];
                A[(size_t)(r1 + i) * nr + r2 + j] = v;
                if (r1 != r2) A[(size_t)(r2 + j) * nr + r1 + i] = v;
            }
    }
    for (int t = 0; t < T; t++)
        if (t != h->anchor)
            for (int i = 0; i < 6; i++) b[ri(t) * 6 + i] = -rhs[t * 6 + i];
    if (nr && !agt_side::cholesky_solve(A, b, nr)) return AGT_CALIB_OK;
    d_tag.assign((size_t)T * 6, 0.0);
    for (int t = 0; t < T; t++)
        if (t != h->anchor)
            for (int i = 0; i < 6; i++) d_tag[t * 6 + i] = b[ri(t) * 6 + i];
    RC(h->dev.upload(h->d_dtag, d_tag.data(), d_tag.size() * sizeof(double)));
    calib_backsub_kernel<<<blocks64(h->F), 64, 0, h->dev.stream>>>(h->P, h->d_Y, h->d_xf, h->d_dtag, h->d_frame[s], h->d_dframe, h->d_frame[1 - s]);
    HC(hipGetLastError());
    *solved = true;
    return AGT_CALIB_OK;
}

}  // namespace

extern "C" {

int agt_calib_version(void) { return AGT_CALIB_VERSION; }

int agt_group_calib_default_options(agt_calib_options* o)
{
    if (!o) return AGT_CALIB_ERR_ARG;
    agt_side::lm_default_options(o);
    return AGT_CALIB_OK;
}

int agt_group_calib_destroy(agt_group_calib* h)
{
    if (!h) return AGT_CALIB_OK;
    h->dev.free_all();
    delete h;
    return AGT_CALIB_OK;
}

int agt_group_calib_create(const agt_calib_problem* pr, void* stream, agt_group_calib** out)
{
    if (!out) return AGT_CALIB_ERR_ARG;
    *out = nullptr;
    if (!pr || !pr->K || !pr->tag_sizes) return AGT_CALIB_ERR_ARG;
    const int T = pr->n_tags, F = pr->n_frames, n = pr->n_obs;
    if (T < 1 || T > AGT_CALIB_MAX_TAGS || F < 1 || F > AGT_CALIB_MAX_FRAMES || n < 0 || (long long)n > (long long)T * F) return AGT_CALIB_ERR_ARG;
    if (pr->anchor < 0 || pr->anchor >= T) return AGT_CALIB_ERR_ARG;
    if (n > 0 && (!pr->obs_frame || !pr->obs_tag || !pr->obs_corners)) return AGT_CALIB_ERR_ARG;
    for (int t = 0; t < T; t++) if (!(pr->tag_sizes[t] > 0.0) || !isfinite(pr->tag_sizes[t])) return AGT_CALIB_ERR_ARG;
    const int nd = pr->ndist;
    if (!(nd == 0 || nd == 4 || nd == 5 || nd == 8 || nd == 12 || nd == 14)) return AGT_CALIB_ERR_CAMERA;
    if (nd > 0 && !pr->dist) return AGT_CALIB_ERR_ARG;

    agt_group_calib* h = new (std::nothrow) agt_group_calib();
    if (!h) return AGT_CALIB_ERR_ALLOC;
    h->dev.stream = (hipStream_t)stream; h->T = T; h->F = F; h->n = n; h->anchor = pr->anchor; h->cur = 0;
    // ---- host side: sort by frame (stable), the (tag, frame) table, the refusals -- before any device work
    std::vector<int> fstart(F + 1, 0), obs_of((size_t)T * F, -1), tag_s(n), frame_s(n);
    std::vector<double> corners_s((size_t)n * 8);
    for (int i = 0; i < n; i++) {
        const int f = pr->obs_frame[i], t = pr->obs_tag[i];
        if (f < 0 || f >= F || t < 0 || t >= T) { delete h; return AGT_CALIB_ERR_ARG; }
        fstart[f + 1]++;
    }
    for (int f = 0; f < F; f++) fstart[f + 1] += fstart[f];
    {
        std::vector<int> fill(fstart.begin(), fstart.end() - 1);
        h->perm.assign(n, 0);
        for (int i = 0; i < n; i++) {
            const int f = pr->obs_frame[i], t = pr->obs_tag[i], p = fill[f]++;
            if (obs_of[(size_t)t * F + f] >= 0) { delete h; return AGT_CALIB_ERR_ARG; }
            obs_of[(size_t)t * F + f] = p;
            h->perm[p] = i; tag_s[p] = t; frame_s[p] = f;
            memcpy(&corners_s[(size_t)p * 8], pr->obs_corners + (size_t)i * 8, 8 * sizeof(double));
        }
    }
    int used = 0;
    for (int f = 0; f < F; f++) used += fstart[f + 1] > fstart[f];
    h->n_used_frames = used;
    if (used < 2) { delete h; return AGT_CALIB_ERR_TOO_FEW_FRAMES; }
    {
        std::vector<int> root(T);
        std::vector<char> co((size_t)T * T, 0);
        for (int t = 0; t < T; t++) root[t] = t;
        auto find = [&](int t) { while (root[t] != t) { root[t] = root[root[t]]; t = root[t]; } return t; };
        for (int f = 0; f < F; f++)
            for (int p = fstart[f]; p < fstart[f + 1]; p++)
                for (int q = p + 1; q < fstart[f + 1]; q++) {
                    const int a = tag_s[p], b = tag_s[q];
                    co[(size_t)a * T + b] = co[(size_t)b * T + a] = 1;
                    const int ra = find(a), rb = find(b);
                    if (ra != rb) root[ra < rb ? rb : ra] = ra < rb ? ra : rb;
                }
        const int ra = find(h->anchor);
        for (int t = 0; t < T; t++)
            if (find(t) != ra) { delete h; return AGT_CALIB_ERR_DISCONNECTED; }
        // (a tag that was never observed has no path either; with T = 1 the lone anchor must at least have been seen)
        std::vector<char> seen(T, 0);
        for (int p = 0; p < n; p++) seen[tag_s[p]] = 1;
        for (int t = 0; t < T; t++) if (!seen[t]) { delete h; return AGT_CALIB_ERR_DISCONNECTED; }
        for (int t1 = 0; t1 < T; t1++)
            for (int t2 = t1; t2 < T; t2++)
                if (t1 != h->anchor && t2 != h->anchor && (t1 == t2 || co[(size_t)t1 * T + t2])) { h->pairs.push_back(t1); h->pairs.push_back(t2); }
        h->n_pairs = (int)h->pairs.size() / 2;
    }
    // ---- device side
    int *d_tag_s, *d_frame_s, *d_fstart, *d_obs_of;
    double *d_corners, *d_sizes;
    int rc = AGT_CALIB_OK;
    auto A = [&](void** p, size_t bytes) { if (!rc) rc = h->dev.alloc(p, bytes); };
    const size_t nn = (size_t)n;
    A((void**)&d_tag_s, nn * sizeof(int)); A((void**)&d_frame_s, nn * sizeof(int)); A((void**)&d_fstart, (size_t)(F + 1) * sizeof(int));
    A((void**)&d_obs_of, (size_t)T * F * sizeof(int)); A((void**)&d_corners, nn * 8 * sizeof(double)); A((void**)&d_sizes, (size_t)T * sizeof(double));
    A((void**)&h->d_pairs, h->pairs.size() * sizeof(int)); A((void**)&h->d_fail, sizeof(int)); A((void**)&h->d_cost, sizeof(double));
    A((void**)&h->d_tilt, 18 * sizeof(double));
    for (int s = 0; s < 2; s++) {
        A((void**)&h->set[s].U, nn * 36 * sizeof(double)); A((void**)&h->set[s].W, nn * 36 * sizeof(double)); A((void**)&h->set[s].V, nn * 36 * sizeof(double));
        A((void**)&h->set[s].gf, nn * 6 * sizeof(double)); A((void**)&h->set[s].gt, nn * 6 * sizeof(double));
        A((void**)&h->set[s].res, nn * 8 * sizeof(double)); A((void**)&h->set[s].cost, nn * sizeof(double));
        A((void**)&h->d_tag[s], (size_t)T * 6 * sizeof(double)); A((void**)&h->d_frame[s], (size_t)F * 6 * sizeof(double));
    }
    A((void**)&h->d_Y, nn * 36 * sizeof(double)); A((void**)&h->d_xf, (size_t)F * 6 * sizeof(double));
    A((void**)&h->d_S, (size_t)h->n_pairs * 36 * sizeof(double)); A((void**)&h->d_rhs, (size_t)T * 6 * sizeof(double));
    A((void**)&h->d_dtag, (size_t)T * 6 * sizeof(double)); A((void**)&h->d_dframe, (size_t)F * 6 * sizeof(double));
    if (!rc) rc = h->dev.upload(d_tag_s, tag_s.data(), nn * sizeof(int));
    if (!rc) rc = h->dev.upload(d_frame_s, frame_s.data(), nn * sizeof(int));
    if (!rc) rc = h->dev.upload(d_fstart, fstart.data(), (size_t)(F + 1) * sizeof(int));
    if (!rc) rc = h->dev.upload(d_obs_of, obs_of.data(), (size_t)T * F * sizeof(int));
    if (!rc) rc = h->dev.upload(d_corners, corners_s.data(), nn * 8 * sizeof(double));
    if (!rc) rc = h->dev.upload(d_sizes, pr->tag_sizes, (size_t)T * sizeof(double));
    if (!rc) rc = h->dev.upload(h->d_pairs, h->pairs.data(), h->pairs.size() * sizeof(int));
    CalibDev& P = h->P;
    memset(&P, 0, sizeof(P));
    double m[18];
    if (agt_side::fill_camera(pr->K, pr->dist, nd, P.cam, m)) {
        if (!rc) rc = h->dev.upload(h->d_tilt, m, sizeof(m));
        P.cam.tilt = h->d_tilt;
    }
    P.n = n; P.F = F; P.T = T;
    P.obs_tag = d_tag_s; P.obs_frame = d_frame_s; P.fstart = d_fstart; P.obs_of = d_obs_of; P.obs_c = d_corners; P.sizes = d_sizes;
    if (rc) { agt_group_calib_destroy(h); return rc; }
    *out = h;
    return AGT_CALIB_OK;
}

int agt_group_calib_eval(agt_group_calib* h, const double* tag_poses, const double* frame_poses, double* residuals_out, double* cost_out)
{
    if (!h || !tag_poses || !frame_poses) return AGT_CALIB_ERR_ARG;
    const int s = h->cur;
    RC(h->dev.upload(h->d_tag[s], tag_poses, (size_t)h->T * 6 * sizeof(double)));
    RC(h->dev.upload(h->d_frame[s], frame_poses, (size_t)h->F * 6 * sizeof(double)));
    double cost = 0.0;
    RC(accumulate(h, s, &cost));
    if (cost_out) *cost_out = cost;
    if (residuals_out) {
        std::vector<double> r((size_t)h->n * 8);
        RC(h->dev.download(r.data(), h->set[s].res, r.size() * sizeof(double)));
        for (int p = 0; p < h->n; p++) memcpy(residuals_out + (size_t)h->perm[p] * 8, &r[(size_t)p * 8], 8 * sizeof(double));
    }
    return AGT_CALIB_OK;
}

int agt_group_calib_step(agt_group_calib* h, double lambda, const double* tag_poses, const double* frame_poses, double* d_tags_out, double* d_frames_out)
{
    if (!h || !tag_poses || !frame_poses || !d_tags_out || !d_frames_out || !(lambda >= 0.0) || !isfinite(lambda)) return AGT_CALIB_ERR_ARG;
    const int s = h->cur;
    RC(h->dev.upload(h->d_tag[s], tag_poses, (size_t)h->T * 6 * sizeof(double)));
    RC(h->dev.upload(h->d_frame[s], frame_poses, (size_t)h->F * 6 * sizeof(double)));
    double cost = 0.0;
    RC(accumulate(h, s, &cost));
    std::vector<double> d_tag;
    bool solved = false;
    RC(damped_step(h, s, lambda, d_tag, &solved));
    if (!solved) return AGT_CALIB_ERR_SINGULAR;
    memcpy(d_tags_out, d_tag.data(), d_tag.size() * sizeof(double));
    return h->dev.download(d_frames_out, h->d_dframe, (size_t)h->F * 6 * sizeof(double));
}

int agt_group_calib_solve(agt_group_calib* h, const agt_calib_options* options, double* tag_poses, double* frame_poses, agt_calib_report* report)
{
    if (!h || !tag_poses || !frame_poses) return AGT_CALIB_ERR_ARG;
    agt_calib_options o;
    if (!agt_side::lm_options(options, o)) return AGT_CALIB_ERR_ARG;
    const int T = h->T, F = h->F;
    int s = h->cur;
    std::vector<double> tag(tag_poses, tag_poses + (size_t)T * 6), trial((size_t)T * 6), d_tag;
    RC(h->dev.upload(h->d_tag[s], tag.data(), tag.size() * sizeof(double)));
    RC(h->dev.upload(h->d_frame[s], frame_poses, (size_t)F * 6 * sizeof(double)));
    double cost0 = 0.0;
    RC(accumulate(h, s, &cost0));
    agt_calib_report rep;
    RC(agt_side::lm_solve(o, cost0, 8 * h->n,
        [&](double lambda, double& cost_trial) {
            bool solved = false;
            RC(damped_step(h, s, lambda, d_tag, &solved));
            if (solved) {
                for (size_t i = 0; i < tag.size(); i++) trial[i] = tag[i] + d_tag[i];
                RC(h->dev.upload(h->d_tag[1 - s], trial.data(), trial.size() * sizeof(double)));
                RC(accumulate(h, 1 - s, &cost_trial));
            }
            return AGT_CALIB_OK;
        },
        [&] { tag = trial; s = 1 - s; }, &rep));
    h->cur = s;
    memcpy(tag_poses, tag.data(), tag.size() * sizeof(double));
    RC(h->dev.download(frame_poses, h->d_frame[s], (size_t)F * 6 * sizeof(double)));
    if (report) *report = rep;
    return AGT_CALIB_OK;
}

}  // extern "C"
