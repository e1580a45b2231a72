// agt_model.hip -- libagt_model.so (include/agt_model.h): the dense model's template learned from a recording.
//
// The rule is stated in the header.  Kernels (FP64, no floating-point atomics):
//     model_frames_kernel       one workgroup per used frame of the call: Rodrigues once (R | t, 12 doubles), then one visibility byte
//                               per tag (agt_tag_visible, the tracker's rule) -- per-frame work done once, not once per sample
//     model_accumulate_kernel   one thread owns one sample for the whole call: it loads n, S, S2, rejected once, walks the call's used
//                               frames in order (R | t through scalar loads: the frame index is uniform), and stores its sums once.
//                               A ring of four frames in registers: frame j is folded in, then its slot requests the taps of frame j + 4,
//                               so three frames' loads are in flight behind every fold (one wave per SIMD has nobody else to hide a
//                               miss behind).
//                               frame_obs: ballot + popcount per frame, kept in lanes; one integer atomic instruction per wave and
//                               64 frames.
// Frames with use = 0 never reach the device: the host compacts the call to its used frames.
// The projection, Rodrigues, the camera and the visibility test are the device functions of agt_device.h / agt_pnp_body.h.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>
#include <new>
#include <vector>
#include "agt_pnp_body.h"
#include "agt_side_buffers.h"
#include "../../include/agt_model.h"

// No contraction in this file's own arithmetic: the accumulate kernel holds several inlined copies of the per-frame code (one per slot of
// its read-ahead ring, and those of the ring's first fill), and a frame meets one copy or another depending on how the recording was cut
// into calls.  Which product of a sum of products is fused into the addition is the compiler's choice, copy by copy; with that choice left
// open the sums of nine one-frame calls differed from those of one nine-frame call in the last bits.  Every fused operation below is
// written out.  (agt_project and agt_rodrigues contract inside their own definitions, agt_device.h.)
#pragma clang fp contract(off)

static_assert(AGT_MODEL_OK == agt_side::OK && AGT_MODEL_ERR_ARG == agt_side::ERR_ARG && AGT_MODEL_ERR_ALLOC == agt_side::ERR_ALLOC &&
              AGT_MODEL_ERR_HIP == agt_side::ERR_HIP, "the shared host code returns this library's codes");

namespace {

#define MODEL_BLOCK 64             // one wave per workgroup: at 61,440 samples 960 workgroups spread over all 1024 SIMDs of the chip
#define MODEL_AHEAD 4              // frames whose taps a thread has in flight (profiles/dense_model.md)

struct ModelDev {                  // the uploaded problem and the accumulators (kernel argument, by value)
    AgtCameraHost cam;
    int w, h, T, M;
    double facing, cos_max;
    const float* tag_corners;      // T x 12
    const float* xyz;              // M x 3
    const int* tag;                // M
    int* n; double* S; double* S2; int* rej;                    // the current pass, SoA
    const int* n_r; const double* S_r; const double* S2_r;      // the reference pass (clipped pass only)
    double clip_sigma, sigma_floor;                              // clip_sigma = 0: plain pass
};

struct ModelCall {                 // one accumulate call
    const uint8_t* frames;
    size_t pitch, frame_stride;
    int nu;                        // used frames
    const int* fidx;               // nu: index of the used frame in the call
    const double* pose;            // nu x 6
    double* rt;                    // nu x 12: R (row-major) | t
    uint8_t* vis;                  // nu x T
    int* frame_obs;                // nu
};

__global__ __launch_bounds__(64) void model_frames_kernel(ModelDev P, ModelCall C)
{
    __shared__ double srt[12];
    const int j = blockIdx.x;
    if (threadIdx.x == 0) {
        double p[6], R[9], G[9];
#pragma unroll
        for (int k = 0; k < 6; k++) p[k] = C.pose[j * 6 + k];
        agt_rodrigues<false>(p, R, G);
#pragma unroll
        for (int k = 0; k < 9; k++) { srt[k] = R[k]; C.rt[j * 12 + k] = R[k]; }
#pragma unroll
        for (int k = 0; k < 3; k++) { srt[9 + k] = p[3 + k]; C.rt[j * 12 + 9 + k] = p[3 + k]; }
        C.frame_obs[j] = 0;
    }
    __syncthreads();
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = srt[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = srt[9 + k];
    for (int g = threadIdx.x; g < P.T; g += 64) {
        double c;
        C.vis[(size_t)j * P.T + g] = agt_tag_visible<float>(P.tag_corners + g * 12, 4, R, t, P.facing, P.cos_max, c) ? 1 : 0;
    }
}

// what a thread holds of one frame between requesting its taps and folding them in
// (the taps as the loads deliver them, 32 bits each, unpacked when they are folded in: byte fields are packed into one register as soon
// as they arrive, which waits for the loads at the place they are requested)
struct ModelTaps { double a, b; unsigned row0, row1, vis; bool in; };

// the call's read-only tables as the kernel's own restrict-qualified arguments: loads through them are known not to alias the sums the
// kernel stores, so the frame-uniform ones (R | t, the frame's index) become scalar loads on their own counter
struct ModelTabs { const double* rt; const int* fidx; const uint8_t* vis; const uint8_t* frames; };

template <bool DIST>
__device__ __forceinline__ ModelTaps model_fetch(const ModelDev& P, const ModelCall& C, const ModelTabs& B, const AgtCamera& cam, int j, int tag, double X, double Y, double Z)
{
    const double* rt = B.rt + j * 12;              // (uniform: scalar loads)
    double R[9], t[3];
#pragma unroll
    for (int k = 0; k < 9; k++) R[k] = rt[k];
#pragma unroll
    for (int k = 0; k < 3; k++) t[k] = rt[9 + k];
    double u, v;
    agt_project<false, DIST>(cam, R, nullptr, t, X, Y, Z, u, v, nullptr, nullptr);
    const double zc = fma(R[8], Z, fma(R[7], Y, R[6] * X)) + t[2];
    const double fx0 = floor(u), fy0 = floor(v);
    ModelTaps q;
    q.in = zc > 0.0 && fx0 >= 1.0 && fx0 <= (double)(P.w - 3) && fy0 >= 1.0 && fy0 <= (double)(P.h - 3);       // (NaN fails)
    q.a = u - fx0; q.b = v - fy0;
    // branch-free: a sample outside the window reads the frame's first 2 x 2 pixels (w, h >= 4) and ignores them
    const size_t off = q.in ? (size_t)(int)fy0 * C.pitch + (size_t)(int)fx0 : 0;
    const uint8_t* p = B.frames + (size_t)B.fidx[j] * C.frame_stride + off;
    q.vis = B.vis[(size_t)j * P.T + tag];
    unsigned short r0, r1;                          // two pixels of a row in one (unaligned) 16-bit load
    __builtin_memcpy(&r0, p, 2); __builtin_memcpy(&r1, p + C.pitch, 2);
    q.row0 = r0; q.row1 = r1;
    return q;
}

template <bool DIST>
__device__ __forceinline__ void model_walk(const ModelDev& P, const ModelCall& C, const ModelTabs& B, const AgtCamera& cam)
{
    const int i = blockIdx.x * MODEL_BLOCK + threadIdx.x;
    const bool live = i < P.M;
    const int si = live ? i : P.M - 1;             // (every lane walks the loop: the ballot below is taken in uniform control flow)
    const double X = (double)P.xyz[(size_t)si * 3], Y = (double)P.xyz[(size_t)si * 3 + 1], Z = (double)P.xyz[(size_t)si * 3 + 2];
    const int tag = P.tag[si];
    int n = P.n[si], rej = P.rej[si];
    double S = P.S[si], S2 = P.S2[si];
    const bool clipped = P.clip_sigma > 0.0;
    double mean_r = 0.0, gate = 0.0;
    bool has_r = false;
    if (clipped) {
        const int nr = P.n_r[si];
        has_r = nr > 0;
        if (has_r) {
            const double dn = (double)nr;
            mean_r = P.S_r[si] / dn;
            const double var = fma(-mean_r, mean_r, P.S2_r[si] / dn);
            const double sd = sqrt(var > 0.0 ? var : 0.0);
            gate = P.clip_sigma * (sd > P.sigma_floor ? sd : P.sigma_floor);
        }
    }
    // a ring of MODEL_AHEAD frames in registers: frame j is folded in, then its slot requests the taps of frame j + MODEL_AHEAD -- a thread
    // has MODEL_AHEAD - 1 frames' loads in flight behind every fold.  Frames are folded in ascending order whatever the depth (the sums
    // are order-fixed).  No branch in the body: past the end the last frame is requested again and ignored.  A conditional request, or
    // one scheduled in front of its slot's fold, makes the slot's old and new contents live together, and the register copy that
    // resolves it waits for the loads where they are issued (measured: no gain from the ring at all) -- hence the scheduling barriers.
    static_assert(64 % MODEL_AHEAD == 0 && MODEL_BLOCK == 64, "the frame_obs flush below assumes both");
    ModelTaps ring[MODEL_AHEAD];
    int fobs = 0;
    const int last = C.nu - 1;
#pragma unroll
    for (int d = 0; d < MODEL_AHEAD; d++) ring[d] = model_fetch<DIST>(P, C, B, cam, d < last ? d : last, tag, X, Y, Z);
    for (int j0 = 0; j0 < C.nu; j0 += MODEL_AHEAD) {
#pragma unroll
        for (int d = 0; d < MODEL_AHEAD; d++) {
            const int j = j0 + d;
            const bool obs = live && j < C.nu && ring[d].in && ring[d].vis != 0;
            const double a = ring[d].a, b = ring[d].b;
            const double p00 = (double)(ring[d].row0 & 255u), p10 = (double)(ring[d].row0 >> 8), p01 = (double)(ring[d].row1 & 255u), p11 = (double)(ring[d].row1 >> 8);
            const double I = fma(a * b, p11, fma((1.0 - a) * b, p01, fma(a * (1.0 - b), p10, (1.0 - a) * (1.0 - b) * p00)));
            const bool keep = obs && (!has_r || fabs(I - mean_r) <= gate);
            if (keep) { n += 1; S += I; S2 = fma(I, I, S2); }
            if (obs && !keep) rej += 1;
            const int cnt = __popcll(__ballot(keep));
            if ((int)threadIdx.x == (j & 63) && j < C.nu) fobs = cnt;
            __builtin_amdgcn_sched_barrier(0);
            const int jn = j + MODEL_AHEAD;
            ring[d] = model_fetch<DIST>(P, C, B, cam, jn < last ? jn : last, tag, X, Y, Z);
            __builtin_amdgcn_sched_barrier(0);
        }
        // frame_obs: lane l holds the wave's count of frame (j0 & ~63) + l; one atomic instruction per 64 frames.  (An atomic per
        // frame in the loop above works against the read-ahead: loads and atomics share one counter, and with an atomic outstanding a
        // wait for a tap becomes a wait for everything; profiles/dense_model.md.)
        if (((j0 + MODEL_AHEAD) & 63) == 0 || j0 + MODEL_AHEAD >= C.nu) {
            const int jf = (j0 & ~63) + (int)threadIdx.x;
            if (jf < C.nu && fobs != 0) atomicAdd(C.frame_obs + jf, fobs);
            fobs = 0;
        }
    }
    if (live) { P.n[i] = n; P.S[i] = S; P.S2[i] = S2; P.rej[i] = rej; }
}

__global__ __launch_bounds__(MODEL_BLOCK) void model_accumulate_kernel(ModelDev P, ModelCall C, const double* __restrict__ rt, const int* __restrict__ fidx,
                                                                       const uint8_t* __restrict__ vis, const uint8_t* __restrict__ frames)
{
    const ModelTabs B = { rt, fidx, vis, frames };
    AgtCamera cam;
    agt_pnp::load_cam<float>(P.cam, cam);
    bool has_dist = false;
#pragma unroll
    for (int k = 0; k < 12; k++) has_dist |= cam.k[k] != 0.0;
    has_dist |= cam.tilt != nullptr;
    if (has_dist) model_walk<true>(P, C, B, cam);
    else model_walk<false>(P, C, B, cam);
}

}  // namespace

struct agt_dense_model {
    AgtSideBuffers dev;
    ModelDev P;
    int *d_n, *d_rej, *d_nr;
    double *d_S, *d_S2, *d_Sr, *d_S2r, *d_tilt;
    // per-call tables, sized for AGT_MODEL_MAX_COUNT frames
    int *d_fidx, *d_fobs;
    double *d_pose, *d_rt;
    uint8_t* d_vis;
    bool pass_open;
    int calls;                     // accumulate calls of the current pass
    long long frames;              // the pass's frame counter
};

extern "C" {

int agt_model_version(void) { return AGT_MODEL_VERSION; }

int agt_dense_model_destroy(agt_dense_model* h)
{
    if (!h) return AGT_MODEL_OK;
    h->dev.free_all();
    delete h;
    return AGT_MODEL_OK;
}

int agt_dense_model_create(const agt_model_problem* pr, void* stream, agt_dense_model** out)
{
    if (!out) return AGT_MODEL_ERR_ARG;
    *out = nullptr;
    if (!pr || !pr->K || !pr->tag_corners || !pr->model_xyz || !pr->sample_tag) return AGT_MODEL_ERR_ARG;
    const int T = pr->n_tags, M = pr->n_samples, w = pr->width, hgt = pr->height;
    if (T < 1 || T > AGT_MODEL_MAX_TAGS || M < 1 || M > AGT_MODEL_MAX_SAMPLES) return AGT_MODEL_ERR_ARG;
    if (w < 4 || w > AGT_MODEL_MAX_SIZE || hgt < 4 || hgt > AGT_MODEL_MAX_SIZE) return AGT_MODEL_ERR_ARG;
    if (!(pr->max_view_deg > 0.0) || !(pr->max_view_deg <= 90.0)) return AGT_MODEL_ERR_ARG;          // (NaN fails)
    if (pr->facing != 1 && pr->facing != -1) return AGT_MODEL_ERR_ARG;
    for (int i = 0; i < M; i++) if (pr->sample_tag[i] < 0 || pr->sample_tag[i] >= T) return AGT_MODEL_ERR_ARG;
    const int nd = pr->ndist;
    if (!(nd == 0 || nd == 4 || nd == 5 || nd == 8 || nd == 12 || nd == 14)) return AGT_MODEL_ERR_CAMERA;
    if (nd > 0 && !pr->dist) return AGT_MODEL_ERR_ARG;

    agt_dense_model* h = new (std::nothrow) agt_dense_model();
    if (!h) return AGT_MODEL_ERR_ALLOC;
    h->dev.stream = (hipStream_t)stream; h->pass_open = false; h->calls = 0; h->frames = 0;
    float *d_corners, *d_xyz;
    int* d_tag;
    int rc = AGT_MODEL_OK;
    auto A = [&](void** p, size_t bytes) { if (!rc) rc = h->dev.alloc(p, bytes); };
    const size_t mm = (size_t)M, cnt = AGT_MODEL_MAX_COUNT;
    A((void**)&d_corners, (size_t)T * 12 * sizeof(float)); A((void**)&d_xyz, mm * 3 * sizeof(float)); A((void**)&d_tag, mm * sizeof(int));
    A((void**)&h->d_n, mm * sizeof(int)); A((void**)&h->d_rej, mm * sizeof(int)); A((void**)&h->d_nr, mm * sizeof(int));
    A((void**)&h->d_S, mm * sizeof(double)); A((void**)&h->d_S2, mm * sizeof(double));
    A((void**)&h->d_Sr, mm * sizeof(double)); A((void**)&h->d_S2r, mm * sizeof(double));
    A((void**)&h->d_tilt, 18 * sizeof(double));
    A((void**)&h->d_fidx, cnt * sizeof(int)); A((void**)&h->d_fobs, cnt * sizeof(int));
    A((void**)&h->d_pose, cnt * 6 * sizeof(double)); A((void**)&h->d_rt, cnt * 12 * sizeof(double));
    A((void**)&h->d_vis, cnt * (size_t)T);
    if (!rc) rc = h->dev.upload(d_corners, pr->tag_corners, (size_t)T * 12 * sizeof(float));
    if (!rc) rc = h->dev.upload(d_xyz, pr->model_xyz, mm * 3 * sizeof(float));
    if (!rc) rc = h->dev.upload(d_tag, pr->sample_tag, mm * sizeof(int));
    ModelDev& P = h->P;
    memset(&P, 0, sizeof(P));
    double m[18];
    if (agt_side::fill_camera(pr->K, pr->dist, nd, P.cam, m)) {
        if (!rc) rc = h->dev.upload(h->d_tilt, m, sizeof(m));
        P.cam.tilt = h->d_tilt;
    }
    P.w = w; P.h = hgt; P.T = T; P.M = M;
    P.facing = (double)pr->facing;
    P.cos_max = pr->max_view_deg == 90.0 ? 0.0 : cos(pr->max_view_deg * (M_PI / 180.0));          // (as agt_tracker_visibility)
    P.tag_corners = d_corners; P.xyz = d_xyz; P.tag = d_tag;
    P.n = h->d_n; P.S = h->d_S; P.S2 = h->d_S2; P.rej = h->d_rej;
    P.n_r = h->d_nr; P.S_r = h->d_Sr; P.S2_r = h->d_S2r;
    if (rc) { agt_dense_model_destroy(h); return rc; }
    *out = h;
    return AGT_MODEL_OK;
}

int agt_dense_model_begin_pass(agt_dense_model* h, double clip_sigma, double sigma_floor)
{
    if (!h || !(clip_sigma >= 0.0) || !isfinite(clip_sigma) || !(sigma_floor >= 0.0) || !isfinite(sigma_floor)) return AGT_MODEL_ERR_ARG;
    const size_t mm = (size_t)h->P.M;
    if (clip_sigma > 0.0) {
        if (!h->pass_open || h->calls < 1) return AGT_MODEL_ERR_ORDER;
        HC(hipMemcpyAsync(h->d_nr, h->d_n, mm * sizeof(int), hipMemcpyDeviceToDevice, h->dev.stream));
        HC(hipMemcpyAsync(h->d_Sr, h->d_S, mm * sizeof(double), hipMemcpyDeviceToDevice, h->dev.stream));
        HC(hipMemcpyAsync(h->d_S2r, h->d_S2, mm * sizeof(double), hipMemcpyDeviceToDevice, h->dev.stream));
    }
    HC(hipMemsetAsync(h->d_n, 0, mm * sizeof(int), h->dev.stream));
    HC(hipMemsetAsync(h->d_rej, 0, mm * sizeof(int), h->dev.stream));
    HC(hipMemsetAsync(h->d_S, 0, mm * sizeof(double), h->dev.stream));
    HC(hipMemsetAsync(h->d_S2, 0, mm * sizeof(double), h->dev.stream));
    HC(hipStreamSynchronize(h->dev.stream));
    h->P.clip_sigma = clip_sigma; h->P.sigma_floor = sigma_floor;
    h->pass_open = true; h->calls = 0; h->frames = 0;
    return AGT_MODEL_OK;
}

int agt_dense_model_accumulate(agt_dense_model* h, const uint8_t* d_frames, size_t pitch, size_t frame_stride, int count,
                               const double* poses, const uint8_t* use, int32_t* frame_obs_out)
{
    if (!h || !d_frames || !poses || count < 1 || count > AGT_MODEL_MAX_COUNT || pitch < (size_t)h->P.w) return AGT_MODEL_ERR_ARG;
    if (!h->pass_open) return AGT_MODEL_ERR_ORDER;
    std::vector<int> fidx;
    std::vector<double> pose;
    for (int f = 0; f < count; f++) {
        if (use && !use[f]) continue;
        for (int k = 0; k < 6; k++) if (!isfinite(poses[(size_t)f * 6 + k])) return AGT_MODEL_ERR_ARG;
        fidx.push_back(f);
        pose.insert(pose.end(), poses + (size_t)f * 6, poses + (size_t)f * 6 + 6);
    }
    const int nu = (int)fidx.size();
    std::vector<int> fobs(nu, 0);
    if (nu) {
        RC(h->dev.upload(h->d_fidx, fidx.data(), (size_t)nu * sizeof(int)));
        RC(h->dev.upload(h->d_pose, pose.data(), (size_t)nu * 6 * sizeof(double)));
        ModelCall C;
        C.frames = d_frames; C.pitch = pitch; C.frame_stride = frame_stride; C.nu = nu;
        C.fidx = h->d_fidx; C.pose = h->d_pose; C.rt = h->d_rt; C.vis = h->d_vis; C.frame_obs = h->d_fobs;
        model_frames_kernel<<<nu, 64, 0, h->dev.stream>>>(h->P, C);
        model_accumulate_kernel<<<(h->P.M + MODEL_BLOCK - 1) / MODEL_BLOCK, MODEL_BLOCK, 0, h->dev.stream>>>(h->P, C, C.rt, C.fidx, C.vis, C.frames);
        HC(hipGetLastError());
        HC(hipMemcpyAsync(fobs.data(), h->d_fobs, (size_t)nu * sizeof(int), hipMemcpyDeviceToHost, h->dev.stream));
        HC(hipStreamSynchronize(h->dev.stream));
    }
    h->calls++; h->frames += count;
    if (frame_obs_out) {
        for (int f = 0; f < count; f++) frame_obs_out[f] = 0;
        for (int j = 0; j < nu; j++) frame_obs_out[fidx[j]] = fobs[j];
    }
    return AGT_MODEL_OK;
}

int agt_dense_model_read(agt_dense_model* h, int32_t* n, double* S, double* S2, int32_t* rejected)
{
    if (!h) return AGT_MODEL_ERR_ARG;
    if (!h->pass_open) return AGT_MODEL_ERR_ORDER;
    const size_t mm = (size_t)h->P.M;
    RC(h->dev.download(n, h->d_n, mm * sizeof(int)));
    RC(h->dev.download(S, h->d_S, mm * sizeof(double)));
    RC(h->dev.download(S2, h->d_S2, mm * sizeof(double)));
    return h->dev.download(rejected, h->d_rej, mm * sizeof(int));
}

}  // extern "C"
