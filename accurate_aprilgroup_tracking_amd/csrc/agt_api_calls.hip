// agt_api_calls.hip -- the stateless cv2-shaped calls of the C ABI: pyramids, LK, solvePnP / projectPoints (device and host-array
// forms), dense refinement, the LK residency cap, the XCD tile order.
#include "agt_ctx.h"
#include <string.h>

int agt_xcd_tile_order(int block, int nblocks, int xcds)
{
    const int xs = xcds == 8 ? 3 : xcds == 4 ? 2 : xcds == 2 ? 1 : xcds == 1 ? 0 : -1;
    if (xs < 0 || nblocks <= 0 || (nblocks & (xcds - 1)) || block < 0 || block >= nblocks) return AGT_ERR_ARG;
    return agt_xcd_order(block, nblocks, xs);
}

int agt_pyr_down_u8(agt_ctx* c, const uint8_t* d_src, int sw, int sh, size_t spitch, size_t sbatch,
                    uint8_t* d_dst, size_t dpitch, size_t dbatch, int B)
{
    if (!c || !d_src || !d_dst || sw <= 0 || sh <= 0 || B <= 0) return AGT_ERR_ARG;
    if ((spitch & 3) || (dpitch & 3) || ((uintptr_t)d_src & 3) || ((uintptr_t)d_dst & 3) || (sbatch & 3) || (dbatch & 3)) return AGT_ERR_ARG;
    if (spitch < (size_t)sw || dpitch < (size_t)((sw + 1) / 2)) return AGT_ERR_ARG;
    const AgtLevel src = { d_src, (long)spitch, (long)sbatch, sw, sh }, dst = { d_dst, (long)dpitch, (long)dbatch, (sw + 1) / 2, (sh + 1) / 2 };
    hipError_t e = agt_launch_pyr_down(c->stream, src, dst, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

int agt_pyramid_build(agt_ctx* c, int slot, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B)
{
    if (!c || slot < 0 || slot > 1) return AGT_ERR_ARG;
    // slots 0 / 1 are ring entries of the tracker too: frames still in flight (fused pipeline groups not yet
    // launched, stage kernels on the library's streams) are enqueued / ordered in front of this build first
    int rc = join_pipeline(c);
    if (rc) return rc;
    c->prebuilt_t = -1;
    return pyramid_build_on(c, c->stream, slot, d_frames, pitch, batch_stride, B);
}

// Both pyramids of a frame pair (slot 0 <- d_prev, slot 1 <- d_next) with ONE launch for levels 1 and 2 (round 6).  A batch of cold
// pairs pays two pyramid launches per step otherwise, each a stream of its own length with a ramp and a tail and a kernel boundary
// between them (~2 us between two streaming kernels on one stream): the two-level rolling pass of 2 B images is the same pass, once.
// The geometry of both frames is one (pitch, batch_stride); deeper levels, other windows and small batches fall back to two builds.
int agt_pyramid_build_pair(agt_ctx* c, const uint8_t* d_prev, const uint8_t* d_next, size_t pitch, size_t batch_stride, int B)
{
    if (!c || !d_prev || !d_next) return AGT_ERR_ARG;
    int rc = join_pipeline(c);
    if (rc) return rc;
    c->prebuilt_t = -1;
    const int L = c->eff_max_level;
    bool one = L >= 2 && agt_step_supported(c->cfg.win) && B > 0 && B <= c->cfg.max_streams &&
               !((pitch & 3) || ((uintptr_t)d_prev & 3) || ((uintptr_t)d_next & 3) || (batch_stride & 3) || pitch < (size_t)c->cfg.width);
    AgtStepParams S;
    AgtStepTables T;
    const uint8_t* src[2] = { d_prev, d_next };
    if (one) {
        memset(&S, 0, sizeof(S));
        memset(&T, 0, sizeof(T));
        S.pnp.fault = c->fault_dev;
        uintptr_t src_align = 0, dst_align = 0;
        for (int k = 0; k < 2; k++) {
            T.pyr_src[0][k] = src[k]; T.pyr_dst[0][k] = c->lmem[k][1]; T.pyr_dst[1][k] = c->lmem[k][2];
            src_align |= (uintptr_t)src[k]; dst_align |= (uintptr_t)c->lmem[k][1] | (uintptr_t)c->lmem[k][2];
        }
        AgtLevel lv[AGT_MAX_LEVELS];
        fill_levels(c, 0, lv);
        lv[0].ptr = d_prev; lv[0].pitch = (long)pitch; lv[0].bstride = (long)batch_stride;
        AgtPyrArgs A[2];
        agt_pyr2_args(lv, B, A);
        A[1].src = nullptr; A[1].dst = nullptr;              // (per frame: the tables)
        agt_pyr2_plan(A, src_align, dst_align, 2);
        one = agt_pyr_rolling(A[0]) || B <= AGT_PYR2_MAX_B;             // (rolling form for big batches; the tiled two-level pass for small ones)
        if (one) {
            agt_step_set_two_level(S, A);
            S.pyr_nf[0] = 2;
            S.n_pyr[0] = agt_pyr_blocks(A[0]) * B * 2;
        }
    }
    if (!one) {
        rc = pyramid_build_on(c, c->stream, 0, d_prev, pitch, batch_stride, B);
        return rc ? rc : pyramid_build_on(c, c->stream, 1, d_next, pitch, batch_stride, B);
    }
    hipError_t e = agt_launch_step(c->stream, S, T, c->cfg.win, AGT_STEP_PYR);
    if (e != hipSuccess) return hip_fail(c, e);
    for (int k = 0; k < 2; k++) {
        RingFrame& f = c->frame[k]; f.ptr = src[k]; f.pitch = (long)pitch; f.bstride = (long)batch_stride;      // (as pyramid_build_on: state_out stays)
        rc = pyramid_levels_on(c, c->stream, k, 3, B);
        if (rc) return rc;
        f.B = B;
    }
    return AGT_OK;
}

int agt_pyramid_max_level(const agt_ctx* c) { return c ? c->eff_max_level : AGT_ERR_ARG; }

int agt_pyramid_level(const agt_ctx* c, int slot, int level, const uint8_t** d_ptr,
                      int* w, int* h, size_t* pitch, size_t* batch_stride)
{
    if (!c || slot < 0 || slot >= c->ring || level < 0 || level > c->eff_max_level) return AGT_ERR_ARG;
    if (c->frame[slot].B <= 0) return AGT_ERR_STATE;
    if (d_ptr) *d_ptr = level == 0 ? c->frame[slot].ptr : c->lmem[slot][level];
    if (w) *w = c->lw[level];
    if (h) *h = c->lh[level];
    if (pitch) *pitch = (size_t)(level == 0 ? c->frame[slot].pitch : c->lpitch[level]);
    if (batch_stride) *batch_stride = (size_t)(level == 0 ? c->frame[slot].bstride : level_bstride(c, level));
    return AGT_OK;
}

int agt_lk_track(agt_ctx* c, int prev_slot, int next_slot,
                 const float* d_prev_pts, float* d_next_pts, uint8_t* d_status, float* d_err,
                 int n, int B, int crit_type, int crit_max_count, double crit_eps,
                 int flags, double min_eig_threshold)
{
    if (!c || prev_slot < 0 || prev_slot > 1 || next_slot < 0 || next_slot > 1) return AGT_ERR_ARG;
    return lk_track_on(c, c->stream, prev_slot, next_slot, d_prev_pts, nullptr, d_next_pts, d_status, d_err, n, B,
                       crit_type, crit_max_count, crit_eps, flags, min_eig_threshold);
}

// agt_lk_track with the forward-backward check: the forward launch as agt_lk_track issues it, then the same kernels back from next_slot
// to prev_slot in verdict mode (agt_tracker_frames.hip lk_verdict_on), on the same stream
int agt_lk_track_fb(agt_ctx* c, int prev_slot, int next_slot, const float* d_prev_pts, float* d_next_pts,
                    uint8_t* d_status, float* d_err, float* d_fb_dist, int n, int B,
                    int crit_type, int crit_max_count, double crit_eps, int flags, double min_eig_threshold, double fb_max_px)
{
    if (!c || prev_slot < 0 || prev_slot > 1 || next_slot < 0 || next_slot > 1) return AGT_ERR_ARG;
    if (!(fb_max_px > 0.0) || !(fb_max_px <= 3.0e38)) return AGT_ERR_ARG;             // (NaN fails both; beyond float32: infinite)
    int rc = lk_track_on(c, c->stream, prev_slot, next_slot, d_prev_pts, nullptr, d_next_pts, d_status, d_err, n, B,
                         crit_type, crit_max_count, crit_eps, flags, min_eig_threshold);
    if (rc) return rc;
    return lk_verdict_on(c, c->stream, prev_slot, next_slot, d_prev_pts, d_next_pts, d_status, d_err, d_fb_dist, n, B,
                         crit_type, crit_max_count, crit_eps, flags, min_eig_threshold, fb_max_px);
}

// the plain solve (no tracker state) on B streams of n points; the caller fills in the camera
static AgtPnpParams plain_solve(const void* obj, long obj_bstride, const void* img, const uint8_t* mask, int dtype, int n,
                                int use_guess, double* pose, int32_t* info, double* err)
{
    AgtPnpParams p;
    memset(&p, 0, sizeof(p));
    p.obj = obj; p.obj_bstride = obj_bstride; p.img = img; p.mask = mask; p.dtype = dtype;
    p.n = n; p.use_guess = use_guess ? 1 : 0; p.pose = pose; p.info = info; p.err = err;
    p.gate_px = 2.0;
    return p;
}

int agt_solve_pnp(agt_ctx* c, const void* d_obj, size_t obj_batch_stride, const void* d_img, int dtype,
                  const uint8_t* d_mask, int n, int B,
                  const double* K, const double* dist, int ndist,
                  double* d_pose, int use_guess, int32_t* d_info, double* d_err)
{
    if (!c || !d_obj || !d_img || !d_pose || B <= 0) return AGT_ERR_ARG;
    if (dtype != AGT_F32 && dtype != AGT_F64) return AGT_ERR_ARG;
    if (n < 3 || n > 256) return AGT_ERR_NPOINTS;
    if (!use_guess && n < 4) return AGT_ERR_NPOINTS;
    AgtPnpParams p = plain_solve(d_obj, (long)obj_batch_stride, d_img, d_mask, dtype, n, use_guess, d_pose, d_info, d_err);
    int rc = camera_on(c, K, dist, ndist, &p.cam);
    if (rc) return rc;
    hipError_t e = agt_launch_pnp(c->stream, p, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

int agt_project_points(agt_ctx* c, const void* d_obj, size_t obj_batch_stride, int dtype, int n, int B,
                       const double* d_pose, const double* K, const double* dist, int ndist,
                       void* d_img_out, double* d_jac)
{
    if (!c || !d_obj || !d_pose || !d_img_out || n <= 0 || B <= 0) return AGT_ERR_ARG;
    if (dtype != AGT_F32 && dtype != AGT_F64) return AGT_ERR_ARG;
    AgtPointsParams p = { d_obj, (long)obj_batch_stride, dtype, n, d_pose };
    int rc = camera_on(c, K, dist, ndist, &p.cam);
    if (rc) return rc;
    p.img_out = d_img_out; p.jac = d_jac;
    hipError_t e = agt_launch_points(c->stream, p, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// the visibility rule of agt_tracker_visibility for B poses: visible_kernel (agt_project.hip), one thread per tag
int agt_tag_visibility(agt_ctx* c, const void* d_obj, size_t obj_batch_stride, int dtype, int n, int B,
                       const double* d_pose, int corners_per_tag, double max_view_deg, int facing,
                       uint8_t* d_visible, double* d_cos)
{
    if (!c || !d_obj || !d_pose || !d_visible || n <= 0 || B <= 0) return AGT_ERR_ARG;
    if (dtype != AGT_F32 && dtype != AGT_F64) return AGT_ERR_ARG;
    if (!visibility_args_ok(corners_per_tag, max_view_deg, facing) || !(max_view_deg > 0.0) || n % corners_per_tag) return AGT_ERR_ARG;
    AgtVisibleParams p = { d_obj, (long)obj_batch_stride, dtype, n, d_pose };
    p.vis_out = d_visible; p.vis_cos = d_cos; p.vis_cos_max = visibility_cos_max(max_view_deg); p.vis_cpt = corners_per_tag; p.vis_facing = facing;
    hipError_t e = agt_launch_visible(c->stream, p, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// the seed rule of agt_tracker_predict for B pairs of poses: flow_kernel (agt_project.hip), one workgroup per stream
int agt_predict_flow(agt_ctx* c, const void* d_obj, size_t obj_batch_stride, int dtype, int n, int B,
                     const double* d_pose_older, const double* d_pose_newer, const double* K, const double* dist, int ndist,
                     const float* d_prev_pts, const uint8_t* d_mask, double max_flow_px,
                     float* d_seed_pts, float* d_flow, float* d_flow_max, double* d_pose_pred)
{
    if (!c || !d_obj || !d_pose_older || !d_pose_newer || !d_prev_pts || !d_seed_pts || n <= 0 || B <= 0) return AGT_ERR_ARG;
    if (dtype != AGT_F32 && dtype != AGT_F64) return AGT_ERR_ARG;
    if (!(max_flow_px > 0.0) || !(max_flow_px <= 1.7976931348623157e308)) return AGT_ERR_ARG;       // (NaN fails both)
    if (n > 256) return AGT_ERR_NPOINTS;
    AgtFlowParams p = { d_obj, (long)obj_batch_stride, dtype, n };
    int rc = camera_on(c, K, dist, ndist, &p.cam);
    if (rc) return rc;
    p.flow_older = d_pose_older; p.flow_newer = d_pose_newer; p.flow_pstride = 6; p.flow_prev = d_prev_pts; p.flow_mask = d_mask;
    p.flow_seed = d_seed_pts; p.flow_out = d_flow; p.flow_max = d_flow_max; p.flow_pred = d_pose_pred; p.flow_cap = (float)max_flow_px;
    hipError_t e = agt_launch_flow(c->stream, p, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// ---- tag consensus (the rule: include/agt_hip.h agt_solve_pnp_consensus).  Three launches on one stream, nothing in between:
//   1. the solver kernels over B * T problems of cpt points (hypothesis launch, agt_kernels.h AgtPnpParams::hyp_T)
//   2. vote_kernel (agt_project.hip), one workgroup per stream: inlier bytes, votes, the winner's pose
//   3. (stateless call) the ordinary masked solve from the winner's pose; (tracker) the unchanged pose step on the smaller mask
int cons_scratch(agt_ctx* c, int B, int T, int n, ConsScratch* s)
{
    const size_t BT = (size_t)B * T;
    const size_t o_info = BT * 6 * sizeof(double), o_win = o_info + BT * 4 * sizeof(int32_t), o_votes = o_win + (size_t)B * 6 * sizeof(double);
    const size_t o_inl = o_votes + (size_t)B * 4 * sizeof(int32_t), need = o_inl + (size_t)B * n;
    if (need > c->cons_cap) {
        hipError_t e = hipStreamSynchronize(c->stream);          // (an earlier call's launches may still read the old block)
        if (e != hipSuccess) return hip_fail(c, e);
        if (c->cons_buf) (void)hipFree(c->cons_buf);
        c->cons_buf = nullptr; c->cons_cap = 0;
        if (hipMalloc((void**)&c->cons_buf, need) != hipSuccess) { hip_fail(c, hipGetLastError()); return AGT_ERR_ALLOC; }
        c->cons_cap = need;
    }
    s->hyp_pose = (double*)c->cons_buf; s->hyp_info = (int32_t*)(c->cons_buf + o_info); s->win = (double*)(c->cons_buf + o_win);
    s->votes = (int32_t*)(c->cons_buf + o_votes); s->inl = (uint8_t*)(c->cons_buf + o_inl);
    return AGT_OK;
}

int consensus_on(agt_ctx* c, hipStream_t stream, const void* d_obj, long obj_bstride, const void* d_img, int dtype, const uint8_t* d_mask,
                 int n, int B, const AgtCameraHost& cam, const double* d_start, int use_guess, const AgtTrackState* track,
                 int cpt, double inlier_px, int min_inliers, uint8_t* d_inl, int32_t* d_votes, double* d_win, ConsScratch* s)
{
    const int T = n / cpt;
    int rc = cons_scratch(c, B, T, n, s);
    if (rc) return rc;
    // a problem that ends early writes no pose: all-ones bytes are NaN poses and flags with every bit set, which the vote discards
    hipError_t e = hipMemsetAsync(s->hyp_pose, 0xff, (size_t)B * T * (6 * sizeof(double) + 4 * sizeof(int32_t)), stream);
    if (e != hipSuccess) return hip_fail(c, e);
    AgtPnpParams h;
    memset(&h, 0, sizeof(h));
    h.cam = cam; h.obj = d_obj; h.obj_bstride = obj_bstride; h.img = d_img; h.mask = d_mask; h.dtype = dtype;
    h.n = cpt; h.use_guess = use_guess ? 1 : 0; h.pose = s->hyp_pose; h.info = s->hyp_info; h.gate_px = 2.0;
    h.hyp_T = T; h.hyp_pose = use_guess ? d_start : nullptr; h.hyp_track = track; h.enhance_ape = c->opt.enhance_ape;
    e = agt_launch_pnp(stream, h, B * T);
    if (e != hipSuccess) return hip_fail(c, e);
    AgtVoteParams v = { d_obj, obj_bstride, dtype, n, cam };
    v.vote_img = d_img; v.vote_mask = d_mask; v.vote_pose = s->hyp_pose; v.vote_info = s->hyp_info;
    v.vote_inl = d_inl ? d_inl : s->inl; v.vote_votes = d_votes ? d_votes : s->votes; v.vote_win = d_win ? d_win : s->win;
    v.vote_tau2 = inlier_px * inlier_px; v.vote_cpt = cpt; v.vote_min = min_inliers;
    e = agt_launch_vote(stream, v, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

int agt_solve_pnp_consensus(agt_ctx* c, const void* d_obj, size_t obj_batch_stride, const void* d_img, int dtype,
                            const uint8_t* d_mask, int n, int B, const double* K, const double* dist, int ndist,
                            double* d_pose, int use_guess, int corners_per_tag, double inlier_px, int min_inliers,
                            uint8_t* d_inliers, int32_t* d_votes, int32_t* d_info, double* d_err)
{
    if (!c || !d_obj || !d_img || !d_pose || !d_inliers || B <= 0 || n <= 0) return AGT_ERR_ARG;
    if (dtype != AGT_F32 && dtype != AGT_F64) return AGT_ERR_ARG;
    if (!(inlier_px > 0.0) || !(inlier_px <= 1.0e150)) return AGT_ERR_ARG;             // (NaN fails both; the square stays finite)
    if (corners_per_tag < 4 || n % corners_per_tag || min_inliers < corners_per_tag) return AGT_ERR_ARG;
    if (n > 256 || n / corners_per_tag > 64) return AGT_ERR_NPOINTS;
    // the refit: agt_solve_pnp(mask = inliers, use_guess = 1).  A stream without consensus has an all-zero mask: pose untouched, info TOO_FEW
    AgtPnpParams p = plain_solve(d_obj, (long)obj_batch_stride, d_img, d_inliers, dtype, n, 1, d_pose, d_info, d_err);
    int rc = camera_on(c, K, dist, ndist, &p.cam);
    if (rc) return rc;
    ConsScratch s;
    // (with a guess the hypotheses start from d_pose, which the vote then overwrites with the winner's pose: same stream, in order)
    rc = consensus_on(c, c->stream, d_obj, (long)obj_batch_stride, d_img, dtype, d_mask, n, B, p.cam, d_pose, use_guess, nullptr,
                      corners_per_tag, inlier_px, min_inliers, d_inliers, d_votes, d_pose, &s);
    if (rc) return rc;
    hipError_t e = agt_launch_pnp(c->stream, p, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// ---- the reference's per-frame calls as ONE synchronous call each, host arrays in and out (detect_pose.py:509-526 solvePnP,
// :441-465 projectPoints).  No copies are enqueued: the arguments go into a host-mapped staging area of the
// context, the kernel reads them and writes its results there over PCIe and stores a sequence word behind them (system scope), the
// calling thread polls the word.  Against upload + launch + download + stream wait (44 / 28 us per call): see DESIGN.md section 6.
namespace {
constexpr size_t HC_SEQ = 0, HC_POSE = 64, HC_INFO = 128, HC_ERR = 144, HC_OBJ = 256, HC_IMG = HC_OBJ + 256 * 3 * 8,
                 HC_JAC = HC_IMG + 256 * 2 * 8, HC_SIZE = HC_JAC + 2 * 256 * 6 * 8;

int hcall_ready(agt_ctx* c)
{
    if (c->hcall_host) return AGT_OK;
    if (hipHostMalloc((void**)&c->hcall_host, HC_SIZE, hipHostMallocMapped) != hipSuccess) { (void)hipGetLastError(); c->hcall_host = nullptr; return AGT_ERR_ALLOC; }
    memset(c->hcall_host, 0, HC_SIZE);
    if (hipHostGetDevicePointer((void**)&c->hcall_dev, c->hcall_host, 0) != hipSuccess) {
        (void)hipGetLastError(); (void)hipHostFree(c->hcall_host); c->hcall_host = nullptr; return AGT_ERR_HIP;
    }
    c->hcall_n = 0;
    return AGT_OK;
}

// one host call (after hcall_ready): the call's number goes into the parameters, whose kernel stores it behind its outputs; launch, poll
template <class P, class Launch>
int hcall_run(agt_ctx* c, P& p, Launch launch)
{
    const unsigned long long want = ++c->hcall_n;
    p.host_seq = (unsigned long long*)(c->hcall_dev + HC_SEQ); p.host_seq_base = want;
    hipError_t e = launch(c->stream, p, 1);
    if (e != hipSuccess) return hip_fail(c, e);
    return poll_seq(c, (const volatile unsigned long long*)(c->hcall_host + HC_SEQ), want);
}
}  // namespace

int agt_solve_pnp_host(agt_ctx* c, const void* h_obj, const void* h_img, int dtype, int n,
                       const double* K, const double* dist, int ndist,
                       double* h_pose, int use_guess, int32_t* h_info, double* h_err)
{
    if (!c || !h_obj || !h_img || !h_pose) return AGT_ERR_ARG;
    if (dtype != AGT_F32 && dtype != AGT_F64) return AGT_ERR_ARG;
    if (n < 3 || n > 256) return AGT_ERR_NPOINTS;
    if (!use_guess && n < 4) return AGT_ERR_NPOINTS;
    int rc = hcall_ready(c);
    if (rc) return rc;
    AgtPnpParams p = plain_solve(c->hcall_dev + HC_OBJ, 0, c->hcall_dev + HC_IMG, nullptr, dtype, n, use_guess, (double*)(c->hcall_dev + HC_POSE),
                                 (int32_t*)(c->hcall_dev + HC_INFO), (double*)(c->hcall_dev + HC_ERR));
    rc = camera_on(c, K, dist, ndist, &p.cam);
    if (rc) return rc;
    const size_t es = dtype == AGT_F32 ? 4 : 8;
    memcpy(c->hcall_host + HC_OBJ, h_obj, (size_t)n * 3 * es);
    memcpy(c->hcall_host + HC_IMG, h_img, (size_t)n * 2 * es);
    double* pose = (double*)(c->hcall_host + HC_POSE);
    if (use_guess) memcpy(pose, h_pose, 6 * sizeof(double)); else memset(pose, 0, 6 * sizeof(double));
    rc = hcall_run(c, p, [](hipStream_t s, const AgtPnpParams& q, int B) { return agt_launch_pnp(s, q, B); });
    if (rc) return rc;
    memcpy(h_pose, pose, 6 * sizeof(double));
    if (h_info) memcpy(h_info, c->hcall_host + HC_INFO, 4 * sizeof(int32_t));
    if (h_err) *h_err = *(const double*)(c->hcall_host + HC_ERR);
    return AGT_OK;
}

int agt_project_points_host(agt_ctx* c, const void* h_obj, int dtype, int n, const double* h_pose,
                            const double* K, const double* dist, int ndist, void* h_img_out, double* h_jac)
{
    if (!c || !h_obj || !h_pose || !h_img_out) return AGT_ERR_ARG;
    if (dtype != AGT_F32 && dtype != AGT_F64) return AGT_ERR_ARG;
    if (n <= 0 || n > 256) return AGT_ERR_NPOINTS;          // (one workgroup: the reference projects its 48 .. 240 model corners)
    int rc = hcall_ready(c);
    if (rc) return rc;
    AgtPointsParams p = { c->hcall_dev + HC_OBJ, 0, dtype, n, (const double*)(c->hcall_dev + HC_POSE) };
    rc = camera_on(c, K, dist, ndist, &p.cam);
    if (rc) return rc;
    const size_t es = dtype == AGT_F32 ? 4 : 8;
    memcpy(c->hcall_host + HC_OBJ, h_obj, (size_t)n * 3 * es);
    memcpy(c->hcall_host + HC_POSE, h_pose, 6 * sizeof(double));
    p.img_out = c->hcall_dev + HC_IMG; p.jac = h_jac ? (double*)(c->hcall_dev + HC_JAC) : nullptr;
    rc = hcall_run(c, p, agt_launch_points);
    if (rc) return rc;
    memcpy(h_img_out, c->hcall_host + HC_IMG, (size_t)n * 2 * es);
    if (h_jac) memcpy(h_jac, c->hcall_host + HC_JAC, (size_t)n * 12 * sizeof(double));
    return AGT_OK;
}

// residency cap of the one-wave LK launches: what it does and the library's choice at lk_lds_min (agt_tracker_frames.hip)
int agt_lk_lds_request(int workgroups_per_cu) { return lk_lds_min(workgroups_per_cu); }

int agt_lk_occupancy_cu(agt_ctx* c, int workgroups_per_cu)
{
    if (!c || workgroups_per_cu < -1 || workgroups_per_cu > 32) return AGT_ERR_ARG;
    int rc = join_pipeline(c);
    if (rc) return rc;
    c->lk_cap_cu = workgroups_per_cu;
    return AGT_OK;
}

// the same in waves per SIMD (round 5's entry point): 4 x waves_per_simd workgroups per CU, 0 = no cap
int agt_lk_occupancy(agt_ctx* c, int waves_per_simd)
{
    if (!c || waves_per_simd < 0 || waves_per_simd > 8) return AGT_ERR_ARG;
    return agt_lk_occupancy_cu(c, 4 * waves_per_simd);
}

// dense photometric + geometric pose refinement (semantics: oracle/cv_dense.c / csrc/agt_dense.hip)
int agt_dense_refine(agt_ctx* c, const uint8_t* d_img, size_t pitch, size_t batch_stride, int w, int h,
                     const float* d_model_xyz, const float* d_model_t, int M,
                     const float* d_obj, const float* d_img_pts, const uint8_t* d_mask, int N,
                     const double* K, const double* dist, int ndist,
                     double* d_pose, int B, int iters, double photo_weight, double* d_stats)
{
    if (!c || !d_img || !d_pose || !d_stats || B <= 0 || w < 4 || h < 4 || iters < 0 || iters > 1000) return AGT_ERR_ARG;
    if (M < 0 || N < 0 || (M > 0 && (!d_model_xyz || !d_model_t)) || (N > 0 && (!d_obj || !d_img_pts))) return AGT_ERR_ARG;
    if (M + N == 0 || pitch < (size_t)w || !(photo_weight >= 0.0)) return AGT_ERR_ARG;
    AgtCameraHost cam;
    int rc = camera_on(c, K, dist, ndist, &cam);
    if (rc) return rc;
    rc = dense_scratch(c, agt_dense_doubles(M, B), B);
    if (rc) return rc;
    agt_dense::DenseParams P = dense_params_on(c);
    P.img = d_img; P.pitch = (long)pitch; P.ibatch = (long)batch_stride; P.w = w; P.h = h;
    P.mxyz = d_model_xyz; P.mt = d_model_t; P.M = M; P.obj = d_obj; P.ipts = d_img_pts; P.mask = d_mask; P.N = N;
    P.cam = cam; P.pose = d_pose; P.stats = d_stats; P.photo_weight = photo_weight;
    hipError_t e = agt_launch_dense(c->stream, P, B, iters);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}
