// agt_api_tracker.hip -- the tracker's entry points of the C ABI: reset, the option setters (the options and their rules: agt_ctx.h
// TrackOptions), the pipeline depth, the frame entry points, which pick the launch form (pipelined or serial: agt_tracker_frames.hip),
// joins, rewind and state reads, profiling.  No host<->device copies and no synchronisation on the per-frame
// path; everything is enqueued on the context's stream.
#include "agt_tracker.h"
#include <new>
#include <math.h>

// What the frame entry points ask of their common arguments, in this order (the codes are ABI): context and frames, a tracker that has
// been reset -- with corners to track from (need_tracked) or at all --, its stream count, the frames' geometry.
static int frame_call_ok(const agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B, bool need_tracked)
{
    if (!c || !d_frames) return AGT_ERR_ARG;
    if (need_tracked ? c->trk_ready != 2 : !c->trk_ready) return AGT_ERR_STATE;
    if (B <= 0 || B != c->trk_B) return AGT_ERR_ARG;
    return frame_args_ok(c, d_frames, pitch, batch_stride) ? AGT_OK : AGT_ERR_ARG;
}

// agt_tracker_predict: a new run, or a new setting, has no pose history
static int pred_clear(agt_ctx* c)
{
    if (!c->pred_hist) return AGT_OK;
    hipError_t e = hipMemsetAsync(c->pred_hist, 0, (size_t)c->cfg.max_streams * AGT_PRED_STRIDE * sizeof(double), c->stream);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

int agt_tracker_reset(agt_ctx* c, int slot, const float* d_corners, const float* d_obj, int n, int B,
                      const double* K, const double* dist, int ndist, int enhance_ape)
{
    if (!c || !d_obj || slot < 0 || slot > 1) return AGT_ERR_ARG;
    if (n < 4 || n > c->cfg.max_points) return AGT_ERR_NPOINTS;
    int rc = c->opt.fits_corners(n);      // whole tags under the options in force
    if (rc) return rc;
    if (B <= 0 || B > c->cfg.max_streams) return AGT_ERR_ARG;
    if (d_corners && c->frame[slot].B < B) return AGT_ERR_STATE;
    rc = join_pipeline(c);            // frames of an earlier run still in flight (fused pipeline or library streams)
    if (rc) return rc;
    if (*(volatile int*)c->fault_host) {
        // recovery from a chained-wait give-up: everything in flight has to be over before the fault word is cleared
        hipError_t es = hipStreamSynchronize(c->stream);
        if (es != hipSuccess) return hip_fail(c, es);
        *(volatile int*)c->fault_host = 0;
    }
    rc = camera_on(c, K, dist, ndist, &c->cam, true);
    if (rc) return rc;
    hipError_t e = hipSuccess;
    // the tracker's frame 0 lives in ring entry 0: adopt the caller's slot as pyramid slot 0
    if (d_corners && slot != 0) {
        for (int l = 1; l <= c->eff_max_level; l++) { uint8_t* t = c->lmem[0][l]; c->lmem[0][l] = c->lmem[slot][l]; c->lmem[slot][l] = t; }
        c->frame[0] = c->frame[slot]; c->frame[slot].B = 0;
    }
    if (d_corners) e = hipMemcpyAsync(c->corners[0], d_corners, (size_t)B * n * 2 * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(c->obj, d_obj, (size_t)n * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(c->tstate, 0, (size_t)B * sizeof(AgtTrackState), c->stream);
    for (int s = 0; s < c->ring && e == hipSuccess; s++) e = hipMemsetAsync(c->status[s], 1, (size_t)B * n, c->stream);
    // arrival counters of the chained launches: a run counts n corners per stream-frame, the next run may have other n / B
    if (e == hipSuccess) e = hipMemsetAsync(c->lk_done, 0, (size_t)AGT_RING_MAX * c->cfg.max_streams * sizeof(unsigned), c->stream);
    memset(c->lk_target, 0, sizeof(c->lk_target));
    if (e != hipSuccess) return hip_fail(c, e);
    rc = pred_clear(c);                      // (agt_tracker_predict: a new run has no pose history)
    if (rc) return rc;
    c->prebuilt_t = -1;
    c->hseq_off = c->hseq_last + 1;          // (sequence numbers of agt_track_host_frame stay monotonic across runs)
    c->trk_n = n; c->trk_B = B; c->opt.enhance_ape = enhance_ape ? 1 : 0;
    frame_complete(c, 0);
    c->trk_ready = d_corners ? 2 : 1;
    return AGT_OK;
}

// What every option setter does once its arguments are in range: `set` changes a copy of the options; the options as they would be
// must fit the corner count of a tracker that has one (the refusal's code is the option's: TrackOptions::fits_corners -- the options in
// force fit it, by agt_tracker_reset and by this check, so only a new whole-tag rule can object); frames in flight are issued under
// the old options first.
template <class Set> static int set_options(agt_ctx* c, Set set)
{
    TrackOptions o = c->opt;
    set(o);
    int rc = c->trk_ready ? o.fits_corners(c->trk_n) : AGT_OK;
    if (rc == AGT_OK && (rc = join_pipeline(c)) == AGT_OK) c->opt = o;
    return rc;
}

int agt_tracker_options(agt_ctx* c, int reproject, int min_points, double gate_px)
{
    if (!c || min_points < 6 || min_points > 256 || !(gate_px > 0.0)) return AGT_ERR_ARG;
    return set_options(c, [=](TrackOptions& o) { o.reproject = reproject ? 1 : 0; o.min_points = min_points; o.gate_px = gate_px; });
}

int agt_tracker_tag_gate(agt_ctx* c, int corners_per_tag)
{
    if (!c || (corners_per_tag != 0 && corners_per_tag != 4)) return AGT_ERR_ARG;
    return set_options(c, [=](TrackOptions& o) { o.tag_gate = corners_per_tag; });
}

// Forward-backward check of the tracker's LK (semantics: include/agt_hip.h; the launch form it forces: agt_ctx.h TrackOptions).
int agt_tracker_fb_check(agt_ctx* c, double fb_max_px)
{
    if (!c || !(fb_max_px >= 0.0) || !(fb_max_px <= 3.0e38)) return AGT_ERR_ARG;       // (NaN fails both; beyond float32: infinite)
    return set_options(c, [=](TrackOptions& o) { o.fb_max_px = fb_max_px; });
}

bool visibility_args_ok(int corners_per_tag, double max_view_deg, int facing)
{
    return max_view_deg >= 0.0 && max_view_deg <= 90.0 && (facing == 1 || facing == -1) && corners_per_tag >= 4;       // (NaN fails both comparisons)
}
// (cos(pi / 2) is 6e-17 in double: at 90 degrees the rule is the plain back-face test, n . c < 0)
double visibility_cos_max(double max_view_deg) { return max_view_deg == 90.0 ? 0.0 : cos(max_view_deg * (M_PI / 180.0)); }

// Visibility rule of the reproject refresh (semantics: include/agt_hip.h; device side: agt_device.h agt_tag_visible, the refresh block of
// agt_pnp_body.h; no launch form changes: agt_ctx.h TrackOptions).  Switching it off succeeds whatever the corner count.
int agt_tracker_visibility(agt_ctx* c, int corners_per_tag, double max_view_deg, int facing)
{
    if (!c || !visibility_args_ok(corners_per_tag, max_view_deg, facing)) return AGT_ERR_ARG;
    return set_options(c, [=](TrackOptions& o) { o.vis_deg = max_view_deg; o.vis_cos_max = visibility_cos_max(max_view_deg); o.vis_cpt = corners_per_tag; o.vis_facing = facing; });
}

// Tag consensus in front of the tracker's pose step (semantics: include/agt_hip.h; the launch form it forces: agt_ctx.h TrackOptions).
int agt_tracker_consensus(agt_ctx* c, int corners_per_tag, double inlier_px, int min_inliers)
{
    if (!c || !(inlier_px >= 0.0) || !(inlier_px <= 1.0e150)) return AGT_ERR_ARG;       // (NaN fails both)
    if (corners_per_tag < 4 || corners_per_tag > 64 || min_inliers < corners_per_tag) return AGT_ERR_ARG;      // (the per-stream guess decision is the one-wave solver's)
    return set_options(c, [=](TrackOptions& o) { o.cons_px = inlier_px; o.cons_cpt = corners_per_tag; o.cons_min = min_inliers; });
}

// ---- agt_tracker_predict (semantics: include/agt_hip.h; device side: agt_project.hip flow_stream, the history block: agt_kernels.h AGT_PRED_*).
// Every record-producing pose launch is preceded by ONE launch of flow_kernel (agt_project.hip), which predicts from the stream's two
// newest records, advances the history and leaves the frame's flow word for the pose launch.  (The launch form it forces: agt_ctx.h TrackOptions.)
int agt_tracker_predict(agt_ctx* c, double max_flow_px)
{
    if (!c || !(max_flow_px >= 0.0) || !(max_flow_px <= 1.7976931348623157e308)) return AGT_ERR_ARG;       // (NaN fails both)
    int rc = join_pipeline(c);
    if (rc) return rc;
    if (max_flow_px > 0.0 && !c->pred_hist) {
        const size_t B = (size_t)c->cfg.max_streams, N = (size_t)c->cfg.max_points;
        const size_t o_flow = B * AGT_PRED_STRIDE * sizeof(double), o_back = o_flow + B * N * 2 * sizeof(float);
        char* buf = nullptr;
        if (hipMalloc((void**)&buf, o_back + B * N * 2 * sizeof(float)) != hipSuccess) { hip_fail(c, hipGetLastError()); return AGT_ERR_ALLOC; }
        c->pred_hist = (double*)buf; c->pred_flow = (float*)(buf + o_flow); c->pred_back = (float*)(buf + o_back);
    }
    rc = pred_clear(c);
    if (rc) return rc;
    c->opt.pred_px = max_flow_px;
    return AGT_OK;
}

// depth 0: separate launches per stage, pose complete in stream order.  depth F >= 1: fused software-pipelined
// step that advances every stage by F frames per launch (one launch every F calls of agt_track_frame).
int agt_tracker_pipeline(agt_ctx* c, int depth)
{
    if (!c || depth < 0 || depth > AGT_MAX_GROUP) return AGT_ERR_ARG;
    if (depth && !agt_step_supported(c->cfg.win)) return AGT_ERR_UNSUPPORTED;
    int rc = join_pipeline(c);
    if (rc) return rc;
    c->pipeline = depth ? 1 : 0;
    const int group = depth ? depth : 1;
    if (group != c->group) {
        // every frame <= trk_frame is complete; re-seat the newest one in a ring that fits the new depth
        const int want = (c->eff_max_level + 2) * group > AGT_SLOTS ? (c->eff_max_level + 2) * group : AGT_SLOTS;
        const int live_ring = c->live_ring;
        rc = ensure_ring(c, want);
        if (rc) return rc;
        if (c->trk_ready == 2) ring_move(c, c->trk_frame, live_ring, want);
        c->live_ring = want;
        c->group = group;
    }
    return AGT_OK;
}

int agt_tracker_join(agt_ctx* c)
{
    if (!c) return AGT_ERR_ARG;
    int rc = join_pipeline(c);
    // (enqueue only: a give-up of a chained wait is reported once the device has written the word -- by the next
    // agt_synchronize at the latest; the flagged records say which frames)
    if (rc == AGT_OK && *(volatile int*)c->fault_host) rc = AGT_ERR_CHAIN;
    return rc;
}

int agt_estimate_pose(agt_ctx* c, const float* d_img, const uint8_t* d_mask, int B, double* d_state_out)
{
    if (!c || !d_img) return AGT_ERR_ARG;
    if (!c->trk_ready) return AGT_ERR_STATE;
    if (B <= 0 || B > c->trk_B) return AGT_ERR_ARG;
    int rc = join_pipeline(c);            // state updates of frames in flight come first
    if (rc) return rc;
    AgtPnpParams p;
    fill_estimate(c, &p, d_img, d_mask, d_state_out, nullptr);
    return pose_step_on(c, c->stream, &p, B, -1);
}

// One frame for B streams.
//   pipeline on  (default, needs reproject == 0): ONE fused launch; frame t's pose is produced
//                 L+1 launches later (or by agt_tracker_join / agt_synchronize).
//   pipeline off : pyrDown.. -> LK -> PnP as separate launches, pose complete in stream order.
int agt_track_frame(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B,
                    double* d_state_out)
{
    int rc = frame_call_ok(c, d_frames, pitch, batch_stride, B, true);
    if (rc) return rc;
    hipEvent_t* pev = profile_events(c);
    // the fused launch pays off while the stages are latency-bound (few streams); the biggest batches fill
    // the chip per stage and run faster as separate launches with their own register budgets
    if (c->pipeline && !c->opt.stage_by_stage() && (agt_step_fits(c->trk_n, B) || !pev)) {
        // fused launch: the three spans collapse into one (span 2 = the whole step_kernel launch)
        if (pev) { (void)hipEventRecord(pev[0], c->stream); (void)hipEventRecord(pev[1], c->stream); (void)hipEventRecord(pev[2], c->stream); }
        rc = step_pipelined(c, d_frames, pitch, batch_stride, B, d_state_out);
        if (pev && rc == AGT_OK) { (void)hipEventRecord(pev[3], c->stream); c->prof_n++; }
        return rc;
    }

    return step_serial(c, d_frames, pitch, batch_stride, B, d_state_out, nullptr, pev);
}

int agt_track_frames(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, size_t frame_stride, int B, int count,
                     double* d_state_out)
{
    if (count < 0 || (frame_stride & 3)) return AGT_ERR_ARG;
    for (int k = 0; k < count; k++) {
        int rc = agt_track_frame(c, d_frames + (size_t)k * frame_stride, pitch, batch_stride, B,
                                 d_state_out ? d_state_out + (size_t)k * B * AGT_STATE_STRIDE : nullptr);
        if (rc) return rc;
    }
    return AGT_OK;
}

// A frame whose corners come from the detector (detect_pose.py:389-437 found >= 2 tags, so the reference does not track):
// the frame joins the stream as frame t (its pyramid is built: the next agt_track_frame tracks FROM it), the supplied table
// becomes the frame's corner set and LK status, and _estimate_pose runs on it -- pyramid pass + one PnP launch, in stream order.
int agt_track_frame_detected(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B,
                             const float* d_corners, const uint8_t* d_mask, double* d_state_out)
{
    if (!c || !d_corners) return AGT_ERR_ARG;
    int rc = frame_call_ok(c, d_frames, pitch, batch_stride, B, false);
    if (rc == AGT_OK) rc = join_pipeline(c);
    if (rc) return rc;
    c->prebuilt_t = -1;
    const long t = c->trk_frame + 1;
    const int slot = ring_slot(c, t);
    rc = pyramid_build_on(c, c->stream, slot, d_frames, pitch, batch_stride, B);
    if (rc) return rc;
    AgtPnpParams p;
    fill_estimate(c, &p, d_corners, d_mask, d_state_out, c->corners[slot], c->status[slot]);
    p.seed_pts = c->corners[slot]; p.seed_status = c->status[slot];
    rc = pose_step_on(c, c->stream, &p, B, -1);
    if (rc) return rc;
    frame_complete(c, t);
    c->trk_ready = 2;
    return AGT_OK;
}

// detect_pose.py:570-574 / the mirror's `if ids:`: a frame in which LK lost EVERY tag does not become the "previous" frame --
// the next frame is tracked from the frame before it, with that frame's corner set and status.  The host sees the record
// (AGT_ST_NTRACK == 0) and takes the frame back: its ring entry is re-used by the next frame, entry t - 1 (never written since)
// is the LK source again.  The pose state machine keeps what the lost frame did to it (guess cleared), as in the reference.
int agt_tracker_rewind(agt_ctx* c)
{
    if (!c) return AGT_ERR_ARG;
    if (c->trk_ready != 2 || c->trk_frame < 1) return AGT_ERR_STATE;
    int rc = join_pipeline(c);
    if (rc) return rc;
    c->prebuilt_t = -1;
    c->trk_frame -= 1;
    c->hseq_off += 1;                         // (the next frame re-uses the frame index: its sequence number must not)
    c->n_lk = c->n_pnp = c->trk_frame;
    for (int s = 0; s < AGT_MAX_LEVELS; s++)
        if (c->n_stage[s] > c->trk_frame) c->n_stage[s] = c->trk_frame;
    return AGT_OK;
}

int agt_tracker_state_size(void) { return (int)sizeof(AgtTrackState); }

int agt_tracker_state_read(agt_ctx* c, void* host_dst, int B)
{
    if (!c || !host_dst || !c->trk_ready || B <= 0 || B > c->trk_B) return AGT_ERR_ARG;
    int rc = join_pipeline(c);
    if (rc) return rc;
    hipError_t e = hipMemcpyAsync(host_dst, c->tstate, (size_t)B * sizeof(AgtTrackState), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// valid after agt_tracker_join: the newest frame's corner set and LK status
int agt_tracker_buffers(const agt_ctx* c, const float** d_corners, const uint8_t** d_status)
{
    if (!c || !c->trk_ready) return AGT_ERR_STATE;
    if (d_corners) *d_corners = c->corners[ring_slot(c, c->trk_frame)];
    if (d_status) *d_status = c->status[ring_slot(c, c->trk_frame)];
    return AGT_OK;
}

// dense stage of the per-frame step (BASELINE configs[4]); semantics in include/agt_hip.h
int agt_tracker_dense(agt_ctx* c, const float* d_model_xyz, const float* d_model_t, int M, int iters, double photo_weight, int reseed)
{
    if (!c || M < 0 || iters < 0 || iters > 1000 || !(photo_weight >= 0.0)) return AGT_ERR_ARG;
    if (M > 0 && (!d_model_xyz || !d_model_t || iters == 0)) return AGT_ERR_ARG;
    int rc = join_pipeline(c);
    if (rc) return rc;
    c->dn_xyz = M ? d_model_xyz : nullptr; c->dn_t = M ? d_model_t : nullptr; c->dn_M = M;
    c->dn_iters = iters; c->dn_weight = photo_weight; c->dn_reseed = reseed ? 1 : 0;
    return AGT_OK;
}

// (One frame: the clip call with count = 1 -- the same checks in the same order, no next frame to ride along, and the flush of a
// deferred dense step in its error path cannot fire, since a step is only ever deferred between two frames of one call.)
int agt_track_frame_dense(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B, double* d_state_out, double* d_dense_out)
{
    return agt_track_frames_dense(c, d_frames, pitch, batch_stride, 0, B, 1, d_state_out, d_dense_out);
}

// `count` consecutive frames of the stream(s), frame k at d_frames + k * frame_stride: agt_track_frame_dense for each, in order.
// Knowing the next frame, the library lets its pyramid pass ride in the current frame's four-wave PnP launch or second dense launch (step_serial) --
// same records, one launch less in every frame's serial chain.
int agt_track_frames_dense(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, size_t frame_stride, int B, int count,
                           double* d_state_out, double* d_dense_out)
{
    if (!c || !d_frames || !d_dense_out || count < 0 || (frame_stride & 3)) return AGT_ERR_ARG;
    int rc = c->opt.dense_refusal();
    // (no dense model and a tracker that has not been reset: the same code)
    if (rc == AGT_OK) rc = c->dn_M <= 0 ? AGT_ERR_STATE : frame_call_ok(c, d_frames, pitch, batch_stride, B, true);
    if (rc) return rc;
    for (int k = 0; k < count; k++) {
        hipEvent_t* pev = profile_events(c);
        rc = step_serial(c, d_frames + (size_t)k * frame_stride, pitch, batch_stride, B,
                         d_state_out ? d_state_out + (size_t)k * B * AGT_STATE_STRIDE : nullptr,
                         d_dense_out + (size_t)k * B * AGT_DENSE_STRIDE, pev, k + 1 < count ? d_frames + (size_t)(k + 1) * frame_stride : nullptr);
        if (rc) {
            if (c->dense_pending) { c->dense_pending = 0; (void)agt_launch_dense_final(c->stream, c->dense_final, B); }     // (a frame failed before its LK launch)
            return rc;
        }
    }
    return AGT_OK;
}

int agt_profile_begin(agt_ctx* c, int max_frames)
{
    if (!c || max_frames <= 0 || max_frames > (1 << 20) || c->prof_ev) return AGT_ERR_ARG;
    const size_t n = (size_t)max_frames * AGT_PROF_EVENTS;
    c->prof_ev = new (std::nothrow) hipEvent_t[n];
    if (!c->prof_ev) return AGT_ERR_ALLOC;
    for (size_t i = 0; i < n; i++) {
        hipError_t e = hipEventCreate(&c->prof_ev[i]);
        if (e != hipSuccess) {
            for (size_t j = 0; j < i; j++) (void)hipEventDestroy(c->prof_ev[j]);
            delete[] c->prof_ev; c->prof_ev = nullptr;
            return hip_fail(c, e);
        }
    }
    c->prof_dense = new (std::nothrow) int[max_frames];
    if (!c->prof_dense) { for (size_t j = 0; j < n; j++) (void)hipEventDestroy(c->prof_ev[j]); delete[] c->prof_ev; c->prof_ev = nullptr; return AGT_ERR_ALLOC; }
    for (int i = 0; i < max_frames; i++) c->prof_dense[i] = 0;
    c->prof_cap = max_frames; c->prof_n = 0;
    return AGT_OK;
}

int agt_profile_end(agt_ctx* c, float* ms_out, int* n_frames)
{
    if (!c || !c->prof_ev) return AGT_ERR_ARG;
    hipError_t e = hipStreamSynchronize(c->stream);
    int rc = e == hipSuccess ? AGT_OK : hip_fail(c, e);
    if (rc == AGT_OK && ms_out)
        for (int f = 0; f < c->prof_n && rc == AGT_OK; f++) {
            hipEvent_t* ev = c->prof_ev + (size_t)f * AGT_PROF_EVENTS;
            for (int k = 0; k < 3; k++) {
                e = hipEventElapsedTime(&ms_out[f * AGT_PROF_SPANS + k], ev[k], ev[k + 1]);
                if (e != hipSuccess) { rc = hip_fail(c, e); break; }
            }
            // dense stage: ev[3] = its start, ev[4] after the last Gauss-Newton launch, ev[5] after the final launch
            float acc = 0.f, upd = 0.f;
            if (c->prof_dense[f] > 0 && rc == AGT_OK) {
                e = hipEventElapsedTime(&acc, ev[3], ev[4]);
                if (e == hipSuccess) e = hipEventElapsedTime(&upd, ev[4], ev[5]);
                if (e != hipSuccess) { rc = hip_fail(c, e); break; }
            }
            ms_out[f * AGT_PROF_SPANS + 3] = acc; ms_out[f * AGT_PROF_SPANS + 4] = upd;
        }
    if (n_frames) *n_frames = c->prof_n;
    for (size_t i = 0; i < (size_t)c->prof_cap * AGT_PROF_EVENTS; i++) (void)hipEventDestroy(c->prof_ev[i]);
    delete[] c->prof_ev; c->prof_ev = nullptr; c->prof_cap = c->prof_n = 0;
    delete[] c->prof_dense; c->prof_dense = nullptr;
    return rc;
}
