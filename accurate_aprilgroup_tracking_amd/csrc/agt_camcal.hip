// agt_camcal.hip -- libagt_camcal.so (include/agt_camcal.h): calibration of the camera from views of a rigid target.
//
// Levenberg-Marquardt over the shared camera vector c[16] and one pose p_v per view with the view poses eliminated.  Per point
// J = [J_c (2 x 16) | J_v (2 x 6)] and, per view, H_v = sum J^T J (22 x 22) = [A_v B_v; B_v^T U_v], g = sum J^T r.  With
// Ad_v = U_v + lambda diag U_v, Y_v = Ad_v^-1 B_v^T (6 x 16), x_v = Ad_v^-1 g_v:
//     S d_c = -(g_c - sum_v B_v x_v),   S = A + lambda diag A - sum_v B_v Y_v,   A = sum_v A_v
//     d_v = -x_v - Y_v d_c
// -- the elimination of agt_calib.hip the other way round: many small per-view blocks against one small dense shared block.
// Kernels (all FP64, every sum in a fixed order -- no floating-point atomics, so a solve is reproducible to the bit):
//     camcal_accumulate_kernel  one wave per view, points in tiles of 64: a lane projects its point and writes its 2 x 23 rows
//                               [J_c | J_v | r] to LDS; then the lanes own the 276 entries of the upper triangle of the view's
//                               23 x 23 block [H g; . r^T r] (at most five each) and sum them over the tile's points in index order
//     camcal_eliminate_kernel   one wave per view: the 6 x 6 LDL^T, Y_v and x_v (one right-hand side per lane), B_v Y_v and B_v x_v
//     camcal_reduce_kernel      S and the right-hand side over the views: 16 fixed segments of views, then the segments in order
//     camcal_backsub_kernel     one thread per view: d_v and the trial pose
//     camcal_cost_kernel        one workgroup: the views' costs (strided, then a fixed tree)
// The reduced system (<= 16 unknowns) is solved on the host by a plain Cholesky over the free entries; the LM loop is host code.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "agt_device.h"
#include "agt_side_buffers.h"
#include "agt_side_device.h"
#include "../../include/agt_camcal.h"

#pragma clang fp contract(fast)

static_assert(AGT_CAMCAL_OK == agt_side::OK && AGT_CAMCAL_ERR_ARG == agt_side::ERR_ARG && AGT_CAMCAL_ERR_ALLOC == agt_side::ERR_ALLOC &&
              AGT_CAMCAL_ERR_HIP == agt_side::ERR_HIP && AGT_CAMCAL_STOP_CONVERGED == agt_side::STOP_CONVERGED &&
              AGT_CAMCAL_STOP_MAX_ITERS == agt_side::STOP_MAX_ITERS && AGT_CAMCAL_STOP_LAMBDA == agt_side::STOP_LAMBDA,
              "the shared host code returns this library's codes");

namespace {

#define CAMCAL_SEGMENTS 16         // camcal_reduce_kernel: waves per workgroup = view segments of the fixed summation tree
#define CAMCAL_NC 16               // camera entries
#define CAMCAL_NJ 22               // columns of J: camera, then the view's pose
#define CAMCAL_NW 23               // ... and the residual as a 23rd column: [J r]^T [J r] holds H, g and r^T r
#define CAMCAL_ROW 47              // doubles per point in LDS: 2 x 23, padded to an odd count (lane stride 94 dwords: conflict-free 8-byte stores)
#define CAMCAL_NE 276              // upper triangle of 23 x 23
#define CAMCAL_RED 272             // entries camcal_reduce_kernel sums: S (16 x 16) and the right-hand side (16)

// index of (i, j), i <= j, in the row-major upper triangle of the 23 x 23 block
__host__ __device__ inline int camcal_tri(int i, int j) { return i * CAMCAL_NW - i * (i - 1) / 2 + (j - i); }

struct CamcalDev {                 // the uploaded problem (kernel argument, by value)
    int V, rsv_;
    const int* vstart;             // V + 1
    const double* X;               // N x 3
    const double* obs;             // N x 2
};

struct CamcalSet {                 // what camcal_accumulate_kernel writes for one camera and set of poses
    double* blk;                   // V x 276: the view's [H g; . r^T r], upper triangle
    double* res;                   // N x 2
    double* cost;                  // V      1/2 sum r^2
};

__global__ __launch_bounds__(64) void camcal_accumulate_kernel(CamcalDev P, AgtCamera cam, const double* __restrict__ pose, CamcalSet S)
{
    __shared__ double rows[64 * CAMCAL_ROW];
    const int v = blockIdx.x, lane = threadIdx.x;
    const int p0 = P.vstart[v], n = P.vstart[v + 1] - p0;
    double pv[6];
#pragma unroll
    for (int i = 0; i < 6; i++) pv[i] = pose[(size_t)v * 6 + i];
    double R[9], G[9];
    agt_rodrigues<true>(pv, R, G);
    const double t[3] = { pv[3], pv[4], pv[5] };
    // the entries this lane owns: e = lane + 64 k
    int ei[5], ej[5];
    double acc[5];
#pragma unroll
    for (int k = 0; k < 5; k++) {
        int rem = lane + 64 * k, i = 0;
        if (rem >= CAMCAL_NE) rem = 0;
        while (rem >= CAMCAL_NW - i) { rem -= CAMCAL_NW - i; i++; }
        ei[k] = i; ej[k] = i + rem; acc[k] = 0.0;
    }
    for (int base = 0; base < n; base += 64) {
        const int cnt = min(64, n - base);
        if (lane < cnt) {
            const size_t p = (size_t)p0 + base + lane;
            const double X = P.X[p * 3], Y = P.X[p * 3 + 1], Z = P.X[p * 3 + 2];
            double u, w, jr[6], jt[6], ju[16], jv[16];
            agt_project<true, true>(cam, R, G, t, X, Y, Z, u, w, jr, jt);
            agt_project_dcam(cam, R, t, X, Y, Z, ju, jv);
            const double ru = u - P.obs[p * 2], rv = w - P.obs[p * 2 + 1];
            S.res[p * 2] = ru; S.res[p * 2 + 1] = rv;
            double* r0 = rows + lane * CAMCAL_ROW;
#pragma unroll
            for (int i = 0; i < CAMCAL_NC; i++) { r0[i] = ju[i]; r0[CAMCAL_NW + i] = jv[i]; }
#pragma unroll
            for (int i = 0; i < 3; i++) {
                r0[CAMCAL_NC + i] = jr[i]; r0[CAMCAL_NC + 3 + i] = jt[i];
                r0[CAMCAL_NW + CAMCAL_NC + i] = jr[3 + i]; r0[CAMCAL_NW + CAMCAL_NC + 3 + i] = jt[3 + i];
            }
            r0[CAMCAL_NJ] = ru; r0[CAMCAL_NW + CAMCAL_NJ] = rv;
        }
        __syncthreads();
        for (int q = 0; q < cnt; q++) {
            const double* r0 = rows + q * CAMCAL_ROW;
#pragma unroll
            for (int k = 0; k < 5; k++) acc[k] += r0[ei[k]] * r0[ej[k]] + r0[CAMCAL_NW + ei[k]] * r0[CAMCAL_NW + ej[k]];
        }
        __syncthreads();
    }
#pragma unroll
    for (int k = 0; k < 5; k++) {
        const int e = lane + 64 * k;
        if (e < CAMCAL_NE) S.blk[(size_t)v * CAMCAL_NE + e] = acc[k];
        if (e == CAMCAL_NE - 1) S.cost[v] = 0.5 * acc[k];
    }
}

// Y: V x 96 [pose parameter][camera entry], xv: V x 6, C: V x 256 = B_v Y_v, rv: V x 16 = B_v x_v
__global__ __launch_bounds__(64) void camcal_eliminate_kernel(CamcalDev P, CamcalSet S, double lambda, double* __restrict__ Y, double* __restrict__ xv,
                                                              double* __restrict__ C, double* __restrict__ rv, int* __restrict__ fail)
{
    __shared__ double sB[CAMCAL_NC][6], sY[CAMCAL_NC + 1][6];
    const int v = blockIdx.x, lane = threadIdx.x;
    const double* H = S.blk + (size_t)v * CAMCAL_NE;
    double A[36];
#pragma unroll
    for (int i = 0; i < 6; i++)
#pragma unroll
        for (int j = 0; j < 6; j++) A[i * 6 + j] = j >= i ? H[camcal_tri(CAMCAL_NC + i, CAMCAL_NC + j)] : 0.0;
#pragma unroll
    for (int i = 0; i < 6; i++) A[i * 7] += lambda * A[i * 7];
    AgtLdl6 F;
    const bool ok = agt_ldl6_factor(A, F);
    if (lane <= CAMCAL_NC) {           // lane c < 16: column c of Y_v (right-hand side: row c of B_v); lane 16: x_v (g_v)
        double b[6], x[6];
#pragma unroll
        for (int k = 0; k < 6; k++) b[k] = lane < CAMCAL_NC ? H[camcal_tri(lane, CAMCAL_NC + k)] : H[camcal_tri(CAMCAL_NC + k, CAMCAL_NJ)];
        agt_ldl6_subst(F, b, x);
#pragma unroll
        for (int k = 0; k < 6; k++) {
            sY[lane][k] = x[k];
            if (lane < CAMCAL_NC) { sB[lane][k] = b[k]; Y[(size_t)v * 96 + k * CAMCAL_NC + lane] = x[k]; }
            else xv[(size_t)v * 6 + k] = x[k];
        }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < 4; q++) {
        const int e = lane + 64 * q, a = e >> 4, b = e & 15;
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += sB[a][k] * sY[b][k];
        C[(size_t)v * 256 + e] = s;
    }
    if (lane < CAMCAL_NC) {
        double s = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) s += sB[lane][k] * sY[CAMCAL_NC][k];
        rv[(size_t)v * CAMCAL_NC + lane] = s;
    }
    if (!ok && lane == 0) *fail = 1;
}

// entry e < 256: S[e / 16][e % 16]; 256 <= e < 272: the right-hand side g_c - sum_v B_v x_v.  The tree depends on V only.
__global__ __launch_bounds__(64 * CAMCAL_SEGMENTS) void camcal_reduce_kernel(CamcalDev P, CamcalSet S, double lambda, const double* __restrict__ C,
                                                                            const double* __restrict__ rv, double* __restrict__ S_out,
                                                                            double* __restrict__ rhs_out)
{
    __shared__ double part[CAMCAL_SEGMENTS][2][64];
    const int l = threadIdx.x & 63, c = threadIdx.x >> 6;
    const int e = blockIdx.x * 64 + l;
    const int per = (P.V + CAMCAL_SEGMENTS - 1) / CAMCAL_SEGMENTS;
    const int v0 = c * per, v1 = min(P.V, v0 + per);
    double a = 0.0, b = 0.0;           // a: A (or g_c), b: B Y (or B x)
    if (e < 256) {
        const int i = min(e >> 4, e & 15), j = max(e >> 4, e & 15), q = camcal_tri(i, j);
        for (int v = v0; v < v1; v++) { a += S.blk[(size_t)v * CAMCAL_NE + q]; b += C[(size_t)v * 256 + e]; }
    } else if (e < CAMCAL_RED) {
        const int i = e - 256, q = camcal_tri(i, CAMCAL_NJ);
        for (int v = v0; v < v1; v++) { a += S.blk[(size_t)v * CAMCAL_NE + q]; b += rv[(size_t)v * CAMCAL_NC + i]; }
    }
    part[c][0][l] = a; part[c][1][l] = b;
    __syncthreads();
    if (c == 0 && e < CAMCAL_RED) {
        double sa = 0.0, sb = 0.0;
        for (int s = 0; s < CAMCAL_SEGMENTS; s++) { sa += part[s][0][l]; sb += part[s][1][l]; }
        if (e < 256) {
            if ((e >> 4) == (e & 15)) sa += lambda * sa;
            S_out[e] = sa - sb;
        } else {
            rhs_out[e - 256] = sa - sb;
        }
    }
}

__global__ __launch_bounds__(64) void camcal_backsub_kernel(CamcalDev P, const double* __restrict__ Y, const double* __restrict__ xv, const double* __restrict__ d_cam,
                                                            const double* __restrict__ pose, double* __restrict__ d_view, double* __restrict__ pose_trial)
{
    const int v = blockIdx.x * 64 + threadIdx.x;
    if (v >= P.V) return;
#pragma unroll
    for (int k = 0; k < 6; k++) {
        double s = 0.0;
#pragma unroll
        for (int j = 0; j < CAMCAL_NC; j++) s += Y[(size_t)v * 96 + k * CAMCAL_NC + j] * d_cam[j];
        const double d = -xv[(size_t)v * 6 + k] - s;
        d_view[(size_t)v * 6 + k] = d;
        pose_trial[(size_t)v * 6 + k] = pose[(size_t)v * 6 + k] + d;
    }
}

__global__ __launch_bounds__(1024) void camcal_cost_kernel(CamcalDev P, const double* __restrict__ cost_v, double* __restrict__ cost_out)
{
    __shared__ double part[1024];
    double acc = 0.0;
    for (int v = threadIdx.x; v < P.V; v += 1024) acc += cost_v[v];
    agt_block_sum_1024(acc, part);
    if (threadIdx.x == 0) cost_out[0] = part[0];
}

AgtCamera make_camera(const double* c)
{
    AgtCamera cam;
    cam.fx = c[0]; cam.fy = c[1]; cam.cx = c[2]; cam.cy = c[3];
    for (int i = 0; i < 12; i++) cam.k[i] = c[4 + i];
    cam.tilt = nullptr;
    return cam;
}

}  // namespace

struct agt_camcal {
    AgtSideBuffers dev;
    CamcalDev P;
    int V, N;
    unsigned free_mask;
    std::vector<int> free_idx;         // the estimated entries of c, ascending
    CamcalSet set[2];
    double* d_pose[2];
    double *d_Y, *d_xv, *d_C, *d_rv, *d_S, *d_rhs, *d_dcam, *d_dview, *d_cost;
    int* d_fail;
    int cur;
};

namespace {

// residuals, the views' blocks and the cost of set s at (camera, d_pose[s])
int accumulate(agt_camcal* h, int s, const double* camera, double* cost)
{
    camcal_accumulate_kernel<<<h->V, 64, 0, h->dev.stream>>>(h->P, make_camera(camera), h->d_pose[s], h->set[s]);
    camcal_cost_kernel<<<1, 1024, 0, h->dev.stream>>>(h->P, h->set[s].cost, h->d_cost);
    HC(hipGetLastError());
    return h->dev.download(cost, h->d_cost, sizeof(double));
}

// the damped step at set s: d_cam (host, 16; exactly 0 for a fixed entry) and, on the device, d_dview and the trial poses in d_pose[1 - s]
int damped_step(agt_camcal* h, int s, double lambda, double* d_cam, bool* solved)
{
    *solved = false;
    HC(hipMemsetAsync(h->d_fail, 0, sizeof(int), h->dev.stream));
    camcal_eliminate_kernel<<<h->V, 64, 0, h->dev.stream>>>(h->P, h->set[s], lambda, h->d_Y, h->d_xv, h->d_C, h->d_rv, h->d_fail);
    camcal_reduce_kernel<<<(CAMCAL_RED + 63) / 64, 64 * CAMCAL_SEGMENTS, 0, h->dev.stream>>>(h->P, h->set[s], lambda, h->d_C, h->d_rv, h->d_S, h->d_rhs);
    HC(hipGetLastError());
    double Sm[256], rhs[CAMCAL_NC];
    int fail = 0;
    HC(hipMemcpyAsync(Sm, h->d_S, sizeof(Sm), hipMemcpyDeviceToHost, h->dev.stream));
    HC(hipMemcpyAsync(rhs, h->d_rhs, sizeof(rhs), hipMemcpyDeviceToHost, h->dev.stream));
    HC(hipMemcpyAsync(&fail, h->d_fail, sizeof(int), hipMemcpyDeviceToHost, h->dev.stream));
    HC(hipStreamSynchronize(h->dev.stream));
    if (fail) return AGT_CAMCAL_OK;
    const int nf = (int)h->free_idx.size();
    std::vector<double> A((size_t)nf * nf), b(nf);
    for (int i = 0; i < nf; i++) {
        b[i] = -rhs[h->free_idx[i]];
        for (int j = 0; j < nf; j++) A[(size_t)i * nf + j] = Sm[h->free_idx[i] * CAMCAL_NC + h->free_idx[j]];
    }
    if (nf && !agt_side::cholesky_solve(A, b, nf)) return AGT_CAMCAL_OK;
    for (int i = 0; i < CAMCAL_NC; i++) d_cam[i] = 0.0;
    for (int i = 0; i < nf; i++) {
        if (!isfinite(b[i])) return AGT_CAMCAL_OK;
        d_cam[h->free_idx[i]] = b[i];
    }
    RC(h->dev.upload(h->d_dcam, d_cam, CAMCAL_NC * sizeof(double)));
    camcal_backsub_kernel<<<(h->V + 63) / 64, 64, 0, h->dev.stream>>>(h->P, h->d_Y, h->d_xv, h->d_dcam, h->d_pose[s], h->d_dview, h->d_pose[1 - s]);
    HC(hipGetLastError());
    *solved = true;
    return AGT_CAMCAL_OK;
}

}  // namespace

extern "C" {

int agt_camcal_version(void) { return AGT_CAMCAL_VERSION; }

int agt_camcal_default_options(agt_camcal_options* o)
{
    if (!o) return AGT_CAMCAL_ERR_ARG;
    agt_side::lm_default_options(o);
    return AGT_CAMCAL_OK;
}

int agt_camcal_destroy(agt_camcal* h)
{
    if (!h) return AGT_CAMCAL_OK;
    h->dev.free_all();
    delete h;
    return AGT_CAMCAL_OK;
}

int agt_camcal_create(const agt_camcal_problem* pr, void* stream, agt_camcal** out)
{
    if (!out) return AGT_CAMCAL_ERR_ARG;
    *out = nullptr;
    if (!pr || !pr->view_start || !pr->object_points || !pr->image_points) return AGT_CAMCAL_ERR_ARG;
    const int V = pr->n_views;
    if (V < 1 || V > AGT_CAMCAL_MAX_VIEWS || pr->view_start[0] != 0 || (pr->free_mask >> CAMCAL_NC)) return AGT_CAMCAL_ERR_ARG;
    for (int v = 0; v < V; v++) {
        const long long nv = (long long)pr->view_start[v + 1] - pr->view_start[v];
        if (nv < AGT_CAMCAL_MIN_VIEW_POINTS || nv > AGT_CAMCAL_MAX_VIEW_POINTS) return AGT_CAMCAL_ERR_ARG;
    }
    const int N = pr->view_start[V];
    const int nd = pr->ndist;
    if (!(nd == 0 || nd == 4 || nd == 5 || nd == 8 || nd == 12)) return AGT_CAMCAL_ERR_CAMERA;
    if (pr->free_mask >> (4 + nd)) return AGT_CAMCAL_ERR_CAMERA;
    int nfree = 0;
    for (int i = 0; i < CAMCAL_NC; i++) nfree += (pr->free_mask >> i) & 1;
    if (2LL * N < 6LL * V + nfree) return AGT_CAMCAL_ERR_TOO_FEW;

    agt_camcal* h = new (std::nothrow) agt_camcal();
    if (!h) return AGT_CAMCAL_ERR_ALLOC;
    h->dev.stream = (hipStream_t)stream; h->V = V; h->N = N; h->free_mask = pr->free_mask; h->cur = 0;
    for (int i = 0; i < CAMCAL_NC; i++) if ((pr->free_mask >> i) & 1) h->free_idx.push_back(i);
    // ---- device side
    int* d_vstart;
    double *d_X, *d_obs;
    int rc = AGT_CAMCAL_OK;
    auto A = [&](void** p, size_t bytes) { if (!rc) rc = h->dev.alloc(p, bytes); };
    const size_t nn = (size_t)N, vv = (size_t)V;
    A((void**)&d_vstart, (vv + 1) * sizeof(int)); A((void**)&d_X, nn * 3 * sizeof(double)); A((void**)&d_obs, nn * 2 * sizeof(double));
    A((void**)&h->d_fail, sizeof(int)); A((void**)&h->d_cost, sizeof(double));
    for (int s = 0; s < 2; s++) {
        A((void**)&h->set[s].blk, vv * CAMCAL_NE * sizeof(double)); A((void**)&h->set[s].res, nn * 2 * sizeof(double));
        A((void**)&h->set[s].cost, vv * sizeof(double)); A((void**)&h->d_pose[s], vv * 6 * sizeof(double));
    }
    A((void**)&h->d_Y, vv * 96 * sizeof(double)); A((void**)&h->d_xv, vv * 6 * sizeof(double));
    A((void**)&h->d_C, vv * 256 * sizeof(double)); A((void**)&h->d_rv, vv * CAMCAL_NC * sizeof(double));
    A((void**)&h->d_S, 256 * sizeof(double)); A((void**)&h->d_rhs, CAMCAL_NC * sizeof(double));
    A((void**)&h->d_dcam, CAMCAL_NC * sizeof(double)); A((void**)&h->d_dview, vv * 6 * sizeof(double));
    if (!rc) rc = h->dev.upload(d_vstart, pr->view_start, (vv + 1) * sizeof(int));
    if (!rc) rc = h->dev.upload(d_X, pr->object_points, nn * 3 * sizeof(double));
    if (!rc) rc = h->dev.upload(d_obs, pr->image_points, nn * 2 * sizeof(double));
    CamcalDev& P = h->P;
    memset(&P, 0, sizeof(P));
    P.V = V; P.vstart = d_vstart; P.X = d_X; P.obs = d_obs;
    if (rc) { agt_camcal_destroy(h); return rc; }
    *out = h;
    return AGT_CAMCAL_OK;
}

int agt_camcal_eval(agt_camcal* h, const double* camera, const double* view_poses, double* residuals_out, double* cost_out)
{
    if (!h || !camera || !view_poses) return AGT_CAMCAL_ERR_ARG;
    const int s = h->cur;
    RC(h->dev.upload(h->d_pose[s], view_poses, (size_t)h->V * 6 * sizeof(double)));
    double cost = 0.0;
    RC(accumulate(h, s, camera, &cost));
    if (cost_out) *cost_out = cost;
    if (residuals_out) RC(h->dev.download(residuals_out, h->set[s].res, (size_t)h->N * 2 * sizeof(double)));
    return AGT_CAMCAL_OK;
}

int agt_camcal_step(agt_camcal* h, double lambda, const double* camera, const double* view_poses, double* d_camera_out, double* d_views_out)
{
    if (!h || !camera || !view_poses || !d_camera_out || !d_views_out || !(lambda >= 0.0) || !isfinite(lambda)) return AGT_CAMCAL_ERR_ARG;
    const int s = h->cur;
    RC(h->dev.upload(h->d_pose[s], view_poses, (size_t)h->V * 6 * sizeof(double)));
    double cost = 0.0, d_cam[CAMCAL_NC];
    RC(accumulate(h, s, camera, &cost));
    bool solved = false;
    RC(damped_step(h, s, lambda, d_cam, &solved));
    if (!solved) return AGT_CAMCAL_ERR_SINGULAR;
    memcpy(d_camera_out, d_cam, sizeof(d_cam));
    return h->dev.download(d_views_out, h->d_dview, (size_t)h->V * 6 * sizeof(double));
}

int agt_camcal_solve(agt_camcal* h, const agt_camcal_options* options, double* camera, double* view_poses, agt_camcal_report* report)
{
    if (!h || !camera || !view_poses) return AGT_CAMCAL_ERR_ARG;
    agt_camcal_options o;
    if (!agt_side::lm_options(options, o)) return AGT_CAMCAL_ERR_ARG;
    const int V = h->V;
    int s = h->cur;
    double cam[CAMCAL_NC], trial[CAMCAL_NC], d_cam[CAMCAL_NC];
    memcpy(cam, camera, sizeof(cam));
    RC(h->dev.upload(h->d_pose[s], view_poses, (size_t)V * 6 * sizeof(double)));
    double cost0 = 0.0;
    RC(accumulate(h, s, cam, &cost0));
    agt_camcal_report rep;
    RC(agt_side::lm_solve(o, cost0, 2 * h->N,
        [&](double lambda, double& cost_trial) {
            bool solved = false;
            RC(damped_step(h, s, lambda, d_cam, &solved));
            if (solved) {
                memcpy(trial, cam, sizeof(cam));        // (a fixed entry is copied, not added to: it keeps its bits, -0.0 included)
                for (int i : h->free_idx) trial[i] = cam[i] + d_cam[i];
                RC(accumulate(h, 1 - s, trial, &cost_trial));
            }
            return AGT_CAMCAL_OK;
        },
        [&] { memcpy(cam, trial, sizeof(cam)); s = 1 - s; }, &rep));
    h->cur = s;
    memcpy(camera, cam, sizeof(cam));
    RC(h->dev.download(view_poses, h->d_pose[s], (size_t)V * 6 * sizeof(double)));
    if (report) *report = rep;
    return AGT_CAMCAL_OK;
}

}  // extern "C"
