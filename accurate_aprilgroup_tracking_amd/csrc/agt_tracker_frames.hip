// agt_tracker_frames.hip -- everything a tracked frame is issued with, in one unit so that the per-frame path stays a chain of static
// functions the compiler sees whole: (1) the stages -- the pyramid of a ring entry, the stand-alone LK launch and its verdict launch
// (also used by the stateless calls, agt_api_calls.hip), the tracker's own LK / seed launches between its ring entries, its pose
// step, the dense stage's scratch; (2) the pipelined launch form (agt_tracker_pipeline depth >= 1): frames are registered in the ring
// and every group launch advances each stage by up to `group` frames -- planned role by role, issued as ONE fused launch or, for big
// batches, in split mode as three launches on the library's streams -- with its drain (join_pipeline) and the move of the live frame
// when the ring size changes; (3) the serial step: pyrDown.. -> LK -> PnP (+ dense stage) as launches on the context's stream, the
// form of depth 0, of every frame while an option forces it (agt_ctx.h TrackOptions::stage_by_stage) and of the dense calls.
#include "agt_tracker.h"

// ---- (1) the stages
int pyramid_build_on(agt_ctx* c, hipStream_t stream, int slot, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B)
{
    if (!c || !d_frames || slot < 0 || slot >= c->ring || B <= 0 || B > c->cfg.max_streams) return AGT_ERR_ARG;
    if (!frame_args_ok(c, d_frames, pitch, batch_stride)) return AGT_ERR_ARG;
    RingFrame& f = c->frame[slot]; f.ptr = d_frames; f.pitch = (long)pitch; f.bstride = (long)batch_stride;       // (B: only once the launches are out)
    AgtLevel lv[AGT_MAX_LEVELS];
    fill_levels(c, slot, lv);
    int l0 = 1;
    if (c->eff_max_level >= 2) {
        // levels 1 and 2 in one pass: level 0 is read once, level 1 is never re-read from HBM.  Big batches: only in the pass's
        // register-rolling form (the tiled one loses to two single passes there)
        AgtPyrArgs A[2];
        agt_pyr2_args(lv, B, A);
        agt_pyr2_plan(A, (uintptr_t)lv[0].ptr, (uintptr_t)lv[1].ptr | (uintptr_t)lv[2].ptr, 1);
        if (B <= AGT_PYR2_MAX_B || agt_pyr_rolling(A[0])) {
            hipError_t e = agt_launch_pyr_down2(stream, A);
            if (e != hipSuccess) return hip_fail(c, e);
            l0 = 3;
        }
    }
    int rc = pyramid_levels_on(c, stream, slot, l0, B);
    if (rc) return rc;
    f.B = B;
    return AGT_OK;
}

int pyramid_levels_on(agt_ctx* c, hipStream_t stream, int slot, int l0, int B)
{
    AgtLevel lv[AGT_MAX_LEVELS];
    fill_levels(c, slot, lv);
    for (int l = l0; l <= c->eff_max_level; l++) {
        hipError_t e = agt_launch_pyr_down(stream, lv[l - 1], lv[l], B);
        if (e != hipSuccess) return hip_fail(c, e);
    }
    return AGT_OK;
}

void fill_levels(const agt_ctx* c, int slot, AgtLevel* L)
{
    for (int l = 0; l <= c->eff_max_level; l++) {
        L[l].w = c->lw[l]; L[l].h = c->lh[l]; L[l].ptr = level_ptr(c, slot, l);
        if (l == 0) { L[l].pitch = c->frame[slot].pitch; L[l].bstride = c->frame[slot].bstride; }
        else { L[l].pitch = c->lpitch[l]; L[l].bstride = level_bstride(c, l); }
    }
}

static int fill_lk(const agt_ctx* c, AgtLkParams* p, int prev_slot, int next_slot, const float* d_prev, const uint8_t* d_prev_status, float* d_next,
                   uint8_t* d_status, float* d_err, int n, int crit_type, int crit_max_count, double crit_eps,
                   int flags, double min_eig_threshold)
{
    memset(p, 0, sizeof(*p));
    fill_levels(c, prev_slot, p->prev);
    fill_levels(c, next_slot, p->next);
    p->max_level = c->eff_max_level;
    p->n = n;
    // SparsePyrLKOpticalFlowImpl::calc criteria normalisation
    p->max_count = (crit_type & AGT_TERM_COUNT) ? (crit_max_count < 0 ? 0 : crit_max_count > 100 ? 100 : crit_max_count) : 30;
    double eps = (crit_type & AGT_TERM_EPS) ? (crit_eps < 0. ? 0. : crit_eps > 10. ? 10. : crit_eps) : 0.01;
    p->eps2 = eps * eps;
    p->flags = flags;
    p->min_eig_threshold = min_eig_threshold;
    p->prev_pts = d_prev; p->prev_status = d_prev_status; p->next_pts = d_next; p->status = d_status; p->err = d_err;
    p->lds_min = lk_lds_min(c->lk_cap_cu > 0 ? c->lk_cap_cu : 0);
    return AGT_OK;
}

// the tracker's own LK from the frame in ring entry prev_slot to the one in `slot`: their corner / status entries, the tracker's criteria
// (flags: AGT_LK_USE_INITIAL_FLOW when the frame's corner entry holds the seeds of agt_tracker_predict, else 0)
static void fill_tracker_lk(const agt_ctx* c, AgtLkParams* p, int prev_slot, int slot, int flags = 0)
{
    fill_lk(c, p, prev_slot, slot, c->corners[prev_slot], c->status[prev_slot], c->corners[slot], c->status[slot], nullptr, c->trk_n,
            AGT_TERM_COUNT | AGT_TERM_EPS, c->lk_max_count, c->lk_eps, flags, c->lk_min_eig);
}

// image k of an LK group per level (k = 0: frame f0, the one before the group) and the corner / status entries of frames f0 + 1 .. f0 + count
static void fill_lk_table(const agt_ctx* c, AgtLkTables& t, long f0, int count)
{
    for (int k = 0; k <= count; k++) {
        const int q = ring_slot(c, f0 + k);
        for (int l = 0; l <= c->eff_max_level; l++) t.img[k][l] = level_ptr(c, q, l);
        if (k) { t.next[k - 1] = c->corners[q]; t.status[k - 1] = c->status[q]; }
    }
}

// Residency cap of the one-wave-per-corner LK kernel (big batches): at most `workgroups_per_cu` of its waves resident on a CU (0 = no// cap: as many as registers and LDS allow, 14-16; -1 = the library's choice, the default).  For launches that SHARE the device with
// other kernels: a tracker wave holds 112 registers and ~7.5 KB of LDS, twelve of them on a CU leave one wave slot of registers per SIMD
// to anybody else, and a launch lasts as long as its slowest corner -- the HBM-bound pyramid passes beside it starve.  The cap is
// enforced with LDS: every workgroup (one wave) asks for at least LDS_per_CU / workgroups_per_cu bytes (more than its tiles need).
// The library's choice: none for a launch of its own (agt_lk_track, the fused step); AGT_SPLIT_LK_CU for the half-batch launches of the
// split pipeline, which run beside the pyramid launch of the frames ahead (round 6, 64 streams of 48 corners: 12 per CU -- all 3,072
// corners resident, the LK launch alone 30.8 us -- step 39.5-40.2 us; 11: 39.1; 10: 38.4; 9: 38.7-39.5; 8: 40.1 -- with 10 the launch alone
// takes 41 us, the step is the shortest; gpurun_out/r6s, profiles/r06_experiments.md).
int lk_lds_min(int per_cu)
{
    if (per_cu <= 0) return 0;
    // The LDS allocation granule is not documented (measured: 12,800 B -> 12 per CU, 13,824 B -> 11: consistent with 512, 1,024 and
    // 1,280 B), so the request is the smallest multiple of 256 B above AGT_LDS_PER_CU / (per_cu + 1): per_cu + 1 workgroups do not fit WHATEVER the granule
    // ("at most per_cu"), and per_cu do fit for granules up to 512 B (for 1,024 / 1,280 B too at the counts the library itself uses, 8 and
    // 10; at some other counts one fewer would: tests/test_chip.py)
    const long v = (AGT_LDS_PER_CU / (per_cu + 1) / 256 + 1) * 256;
    return v > 64L * 1024 ? 0 : (int)v;                 // (a workgroup may ask for 64 KB in all: one per CU cannot be expressed -- no cap then)
}

#define AGT_SPLIT_LK_CU 10       // (see agt_lk_occupancy_cu)
// The stand-alone LK launch of a filled parameter block.  b0: first stream of the launch (streams b0 .. b0 + B - 1 of the slots and of
// the point arrays); waves: see agt_launch_lk
static int lk_launch_on(agt_ctx* c, hipStream_t stream, AgtLkParams& p, int prev_slot, int next_slot, int B, int b0, int waves)
{
    if (c->frame[prev_slot].B < b0 + B || c->frame[next_slot].B < b0 + B) return AGT_ERR_STATE;
    // (waves == 1: a half-batch launch of the split pipeline -- beside the other half's launch and the pyramid launch of the frames ahead)
    p.lds_min = lk_lds_min(c->lk_cap_cu >= 0 ? c->lk_cap_cu : (waves == 1 ? AGT_SPLIT_LK_CU : 0));
    if (c->lk_cap_cu > 0) p.flags |= AGT_LK_FLAG_COTENANT;        // (declared by the caller: agt_lk_occupancy_cu; see agt_lk.hip lk_kernel)
    if (b0) {
        const int n = p.n;
        for (int l = 0; l <= c->eff_max_level; l++) { p.prev[l].ptr += (long)b0 * p.prev[l].bstride; p.next[l].ptr += (long)b0 * p.next[l].bstride; }
        p.prev_pts += (size_t)b0 * n * 2; p.next_pts += (size_t)b0 * n * 2; p.status += (size_t)b0 * n;
        if (p.prev_status) p.prev_status += (size_t)b0 * n;
        if (p.err) p.err += (size_t)b0 * n;
        if (p.fb.orig) p.fb.orig += (size_t)b0 * n * 2;
        if (p.fb.dist) p.fb.dist += (size_t)b0 * n;
    }
    hipError_t e = agt_launch_lk(stream, p, c->cfg.win, B, c->cfg.win == 21 ? waves : 0);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

int lk_track_on(agt_ctx* c, hipStream_t stream, int prev_slot, int next_slot,
                const float* d_prev_pts, const uint8_t* d_prev_status, float* d_next_pts, uint8_t* d_status, float* d_err,
                int n, int B, int crit_type, int crit_max_count, double crit_eps,
                int flags, double min_eig_threshold, int b0, int waves)
{
    if (!c || !d_prev_pts || !d_next_pts || !d_status) return AGT_ERR_ARG;
    if (prev_slot < 0 || prev_slot >= c->ring || next_slot < 0 || next_slot >= c->ring) return AGT_ERR_ARG;
    if (n < 0 || B <= 0 || b0 < 0) return AGT_ERR_ARG;
    if (n == 0) return AGT_OK;
    AgtLkParams p;
    fill_lk(c, &p, prev_slot, next_slot, d_prev_pts, d_prev_status, d_next_pts, d_status, d_err, n, crit_type, crit_max_count, crit_eps,
            flags & 0xffff, min_eig_threshold);          // (the bits above 0xffff are internal launch flags)
    return lk_launch_on(c, stream, p, prev_slot, next_slot, B, b0, waves);
}

// The backward launch of the forward-backward check, behind the forward launch prev_slot -> next_slot on the same stream: the same
// kernels from next_slot back to prev_slot, started at the forward result d_next_pts (no initial flow), for the corners the forward pass
// kept (d_status is its prev_status), in verdict mode (agt_kernels.h AgtLkVerdict): it writes no point and no err -- d_err only says
// whether the pass measures one, as the forward pass did, since measuring can drop a corner whose final window left the image -- clears
// the status byte of a corner that does not come home within fb_max_px of d_prev_pts, and files the distances in d_fb_dist (or null).
// d_back_seed (agt_tracker_predict; null otherwise): [B][n][2] points the pass starts its search at instead, as an initial flow.
int lk_verdict_on(agt_ctx* c, hipStream_t stream, int prev_slot, int next_slot,
                  const float* d_prev_pts, const float* d_next_pts, uint8_t* d_status, const float* d_err, float* d_fb_dist,
                  int n, int B, int crit_type, int crit_max_count, double crit_eps,
                  int flags, double min_eig_threshold, double fb_max_px, const float* d_back_seed)
{
    if (!c || !d_prev_pts || !d_next_pts || !d_status || n < 0 || B <= 0) return AGT_ERR_ARG;
    if (n == 0) return AGT_OK;
    AgtLkParams p;
    // (a verdict launch writes no point: next_pts is only ever read, and only under the initial-flow flag)
    fill_lk(c, &p, next_slot, prev_slot, d_next_pts, d_status, const_cast<float*>(d_back_seed ? d_back_seed : d_next_pts), d_status,
            const_cast<float*>(d_err), n, crit_type, crit_max_count, crit_eps,
            (flags & 0xffff & ~AGT_LK_USE_INITIAL_FLOW) | (d_back_seed ? AGT_LK_USE_INITIAL_FLOW : 0), min_eig_threshold);
    p.fb.orig = d_prev_pts; p.fb.dist = d_fb_dist; p.fb.max_px = (float)fb_max_px;
    return lk_launch_on(c, stream, p, next_slot, prev_slot, B, 0, 0);
}

// the tracker's LK launch of streams b0 .. b0 + B - 1 between two of its ring entries (B >= 1 and trk_n >= 4 by agt_tracker_reset)
static int track_lk_on(agt_ctx* c, hipStream_t stream, int prev_slot, int slot, int B, int b0 = 0, int waves = 0, int flags = 0)
{
    AgtLkParams p;
    fill_tracker_lk(c, &p, prev_slot, slot, flags);
    return lk_launch_on(c, stream, p, prev_slot, slot, B, b0, waves);
}

// prev_slot >= 0: in front of the LK launch prev_slot -> slot -- seeds into the frame's corner entry (mask: the previous frame's LK status),
// flows into the context's scratch.  prev_slot < 0: a frame without an LK step -- the history moves on, the flow word is 0.
static int track_seed_on(agt_ctx* c, hipStream_t stream, int prev_slot, int slot, int B)
{
    AgtFlowParams q = {};
    q.dtype = AGT_F32; q.flow_hist = c->pred_hist; q.flow_cap = (float)c->opt.pred_px;
    if (prev_slot >= 0) {
        q.obj = c->obj; q.n = c->trk_n; q.cam = c->cam;
        q.flow_prev = c->corners[prev_slot]; q.flow_mask = c->status[prev_slot]; q.flow_seed = c->corners[slot]; q.flow_out = c->pred_flow;
    }
    hipError_t e = agt_launch_flow(stream, q, B);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

void fill_estimate(const agt_ctx* c, AgtPnpParams* p, const float* d_img, const uint8_t* d_mask,
                   double* d_state_out, float* corners_rw, uint8_t* status_rw)
{
    memset(p, 0, sizeof(*p));
    p->obj = c->obj; p->obj_bstride = 0; p->img = d_img; p->mask = d_mask; p->dtype = AGT_F32;
    p->n = c->trk_n; p->cam = c->cam; p->pose = c->pose;
    p->track = c->tstate; p->state_out = d_state_out; p->corners_rw = corners_rw; p->status_rw = status_rw;
    p->enhance_ape = c->opt.enhance_ape; p->reproject = c->opt.reproject; p->min_points = c->opt.min_points; p->gate_px = c->opt.gate_px;
    p->tag_gate = c->opt.tag_gate; p->fault = c->fault_dev;
    if (c->opt.vis_deg > 0.0) { p->vis_cpt = c->opt.vis_cpt; p->vis_cos_max = c->opt.vis_cos_max; p->vis_facing = c->opt.vis_facing; }
    if (c->opt.pred_px > 0.0) p->pred_hist = c->pred_hist;
}

// the solver of the launch's first frame `frame` (tracker frame index) reports to the polling host thread (agt_track_host_frame)
static void arm_host_seq(agt_ctx* c, AgtPnpParams* p, long frame)
{
    if (!c->host_seq_on) return;
    p->host_seq = c->hseq_dev;
    p->host_seq_base = c->hseq_off + (unsigned long long)frame;
}

// The pose step of a frame on `stream`, filled in `p`: under agt_tracker_predict the seed launch of a frame WITHOUT an LK step
// (prev_slot < 0; a frame tracked from prev_slot had its seed launch in front of the LK launch), under agt_tracker_consensus its
// two launches, then the pose launch (ride: agt_launch_pnp).
int pose_step_on(agt_ctx* c, hipStream_t stream, AgtPnpParams* p, int B, int prev_slot, const AgtPyrArgs* ride)
{
    int rc;
    if (c->opt.pred_px > 0.0 && prev_slot < 0 && (rc = track_seed_on(c, stream, -1, 0, B))) return rc;
    if (c->opt.cons_px > 0.0) {
        // the frame's consensus over the corners the step is about to solve on (p->img, p->mask): two launches, after which the
        // step uses a corner only while it is an inlier as well and reports the winning count
        ConsScratch cs;
        rc = consensus_on(c, stream, c->obj, 0, p->img, AGT_F32, p->mask, c->trk_n, B, c->cam, nullptr, 0, c->tstate,
                          c->opt.cons_cpt, c->opt.cons_px, c->opt.cons_min, nullptr, nullptr, nullptr, &cs);
        if (rc) return rc;
        p->cons_inl = cs.inl; p->cons_votes = cs.votes;
    }
    hipError_t e = agt_launch_pnp(stream, *p, B, ride);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// scratch of the dense refinement: `need` doubles of block partials and one done word per stream; the two
// capacities are tracked separately (a later call may bring more streams with fewer samples)
agt_dense::DenseParams dense_params_on(const agt_ctx* c)
{
    agt_dense::DenseParams P = agt_dense::DenseParams();
    P.partials = c->dense_partials; P.done = c->dense_done; P.mu = 1e-3;
    return P;
}

int dense_scratch(agt_ctx* c, size_t need, int B)
{
    if (need <= c->dense_cap && B <= c->dense_done_B) return AGT_OK;
    hipError_t e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) return hip_fail(c, e);
    if (need > c->dense_cap) {
        if (c->dense_partials) (void)hipFree(c->dense_partials);
        c->dense_partials = nullptr; c->dense_cap = 0;
        if (hipMalloc((void**)&c->dense_partials, need * sizeof(double)) != hipSuccess) { hip_fail(c, hipGetLastError()); return AGT_ERR_ALLOC; }
        c->dense_cap = need;
    }
    if (B > c->dense_done_B) {
        if (c->dense_done) (void)hipFree(c->dense_done);
        c->dense_done = nullptr; c->dense_done_B = 0;
        if (hipMalloc((void**)&c->dense_done, (size_t)B * sizeof(int) + 64) != hipSuccess) { hip_fail(c, hipGetLastError()); return AGT_ERR_ALLOC; }
        c->dense_done_B = B;
    }
    return AGT_OK;
}

// ---- (2) the pipelined form
// Big batches: pyramid, LK and PnP of one frame as separate kernels on three library-owned streams.  The host runs
// ahead, so the pyramid of frame t+1 overlaps the LK of frame t and the PnP of frame t-1; every true dependency
// (and every buffer reuse of the rings) is an event wait, nothing is assumed about timing.
static int ms_init(agt_ctx* c)
{
    if (c->ms_ready) return AGT_OK;
    if (c->ms_pool_slot < 0) c->ms_pool_slot = ms_pool_acquire(c->cfg.device, c->ms_stream);        // (a retry after a failed event creation keeps its slot)
    if (c->ms_pool_slot < 0) return hip_fail(c, hipGetLastError());
    for (int k = 0; k < SplitEvents::ROWS; k++)
        for (int i = 0; i < AGT_EV_SLOTS; i++) {
            hipEvent_t& ev = c->split.ev[k][i];
            if (!ev && hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) { ev = nullptr; return hip_fail(c, hipGetLastError()); }
        }
    c->ms_ready = 1;
    return AGT_OK;
}

// the caller's stream waits for everything in flight on the library's streams (the LK and PnP launches of split mode)
static int ms_join(agt_ctx* c)
{
    if (!c->ms_active) return AGT_OK;
    hipEvent_t* join = c->split.ev[SplitEvents::MISC];
    hipEvent_t ev1 = join[SplitEvents::JOIN_LK], ev2 = join[SplitEvents::JOIN_POSE], ev0 = join[SplitEvents::JOIN_LK2];
    hipError_t e = hipEventRecord(ev1, c->ms_stream[1]);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev1, 0);
    if (e == hipSuccess) e = hipEventRecord(ev0, c->ms_stream[0]);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev0, 0);
    if (e == hipSuccess) e = hipEventRecord(ev2, c->ms_stream[2]);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, ev2, 0);
    if (e != hipSuccess) return hip_fail(c, e);
    c->ms_active = 0;
    c->split.reset_history();            // everything issued so far is ordered before the caller's next work
    return AGT_OK;
}

// ---- One group launch: every pipeline stage advances by up to `group` frames whose input is complete.  launch_group (below) takes
// a snapshot of the pipeline, PLANS the three roles (plan_pyramid, plan_lk, plan_pose: each fills its part of the launch's parameters
// S and per-frame tables T and advances its own counters of the context: n_stage, n_lk, n_pnp + lk_target), and ISSUES the launch
// in the fused or the split form.  Whatever has to be decided on the state BEFORE the launch is decided on the snapshot.
struct GroupEntry {
    int L, F, B;                                 // pyramid stages 0..L-1 (stage s: level s -> s+1); the most frames a role advances by; streams
    // agt_step_fits: the fused launch (one kernel, all roles), otherwise the split form.  The fused launch is also CHAINED: its PnP role
    // follows the LK role of the SAME launch frame by frame through arrival counters (agt_step.hip pnp_role), instead of one launch behind it.
    bool fits;
    // a launch that will carry pyramid work ONLY (the first one of a run: no frame is ready for the LK role, none for the pose role)
    // goes out as the pyramid kernel proper (issue_fused), which has the register-rolling two-level pass -- the fused step kernel has not
    bool pyr_only;
    long done_before[AGT_MAX_LEVELS + 1];        // [s] = frames available as input of stage s (s = L: input of LK)
    long lk_before;                              // frames tracked so far: the LK role's group starts behind this frame
};

// geometry of pyramid stage s (level s -> s + 1); stage 0's source pitch and stream stride are those of the caller's frames
static void stage_geometry(const agt_ctx* c, int s, int B, AgtPyrArgs& A)
{
    A.sw = c->lw[s]; A.sh = c->lh[s]; A.dw = c->lw[s + 1]; A.dh = c->lh[s + 1]; A.B = B;
    if (s) { A.spitch = c->lpitch[s]; A.sbatch = level_bstride(c, s); }
    A.dpitch = c->lpitch[s + 1]; A.dbatch = level_bstride(c, s + 1);
}

#define AGT_SPLIT_PYR_OH 6       // strip height (level-2 rows) of the split pipeline's pyramid role (agt_pyramid.hip agt_pyr2_plan) ...
#define AGT_SPLIT_PYR_OH_B0 12   // ... for batches of 12 .. 96 streams: measured (session r6ar, us per step, strips of 6 / 16) 8 streams 20.1 / 19.8,
#define AGT_SPLIT_PYR_OH_B1 96   // 16: 27.5 / 28.3, 32: 29.4 / 29.9, 64: 35.1-35.9 / 36.7-37.6, 128: 63.7 / 62.4
// Stage 0 as the two-level pass (levels 1 and 2 from level 0; agt_step_set_two_level): the pass's grid is 64 x 16 tiles of level 2
// (tiled form) or workgroups per image with the strip height in strip_rows (register-rolling form, agt_pyramid4_body.h).  Stage 0's
// single-level plan of frames first .. first + cnt - 1 is in S.pyr[0] / T; returns whether the two-level pass replaces it (`fused`
// on entry: it has to, the batch is small).
static bool plan_two_level(agt_ctx* c, const GroupEntry& G, AgtStepParams& S, AgtStepTables& T, long first, int cnt,
                           uintptr_t src_align, uintptr_t dst_align, bool fused)
{
    const int B = G.B;
    AgtPyrArgs A[2] = { S.pyr[0], S.pyr[1] };
    stage_geometry(c, 1, B, A[1]);
    uintptr_t d2_align = 0;
    for (int k = 0; k < cnt; k++) d2_align |= (uintptr_t)c->lmem[ring_slot(c, first + k)][2];
    // (fused step: agt_step_fits, <= 256 corners in flight -- its kernel carries the tiled two-level pass only: plan as ONE frame, which
    // keeps the launch below the rolling form's 16 images.  Round 5: except the pyramid-only launch at the head of a run, which is
    // pyr_group_kernel -- 20 frames of 1280x720, the driver's block: 15.1 us tiled, see DESIGN.md section 6 for the rolling figure)
    agt_pyr2_plan(A, src_align, dst_align | d2_align, (G.fits && !G.pyr_only) ? 1 : cnt,
                  (G.fits || B < AGT_SPLIT_PYR_OH_B0 || B > AGT_SPLIT_PYR_OH_B1) ? 16 : AGT_SPLIT_PYR_OH);
    if (!fused && agt_pyr_rolling(A[0]) && c->n_stage[1] == first - 1) fused = true;       // big batch, rolling form, no backlog (stage 1 is where stage 0 is)
    if (fused) {
        agt_step_set_two_level(S, A);
        for (int k = 0; k < cnt; k++) T.pyr_dst[1][k] = c->lmem[ring_slot(c, first + k)][2];
        c->n_stage[1] += cnt;            // (same frames: level 2 is complete when level 1 is)
    }
    return fused;
}

// Pyramid role: stage s takes up to F of the frames whose level s is complete.  Returns whether any stage has work.
static bool plan_pyramid(agt_ctx* c, const GroupEntry& G, AgtStepParams& S, AgtStepTables& T)
{
    const int L = G.L, B = G.B;
    bool any = false;
    // stage 0 builds levels 1 and 2 in one pass (stage 1 then only keeps the books): always while the batch is small (tiled or
    // register-rolling two-level pass), for big batches where the rolling form applies to every frame of the launch (plan_two_level)
    // and stage 1 has no backlog from an earlier launch that ran the levels as two passes
    bool fused = L >= 2 && B <= AGT_PYR2_MAX_B;
    for (int s = 0; s < L; s++) {
        if (fused && s == 1) continue;
        const long first = c->n_stage[s] + 1;    // the stage's next frame
        long cnt = G.done_before[s] - c->n_stage[s];
        if (cnt <= 0) continue;
        if (cnt > G.F) cnt = G.F;
        AgtPyrArgs& A = S.pyr[s];
        stage_geometry(c, s, B, A);
        uintptr_t src_align = 0, dst_align = 0;
        for (long k = 0; k < cnt; k++) {
            const int slot = ring_slot(c, first + k);
            if (s == 0) {
                // level 0 is the caller's frame: the frames of a group must share pitch and stream stride
                if (k == 0) { A.spitch = c->frame[slot].pitch; A.sbatch = c->frame[slot].bstride; }
                else if (!same_geometry(c->frame[slot], c->frame[ring_slot(c, first)])) { cnt = k; break; }
            }
            T.pyr_src[s][k] = level_ptr(c, slot, s);
            T.pyr_dst[s][k] = c->lmem[slot][s + 1];
            src_align |= (uintptr_t)T.pyr_src[s][k]; dst_align |= (uintptr_t)T.pyr_dst[s][k];
        }
        A.src = T.pyr_src[s][0]; A.dst = T.pyr_dst[s][0];
        agt_pyr_plan(&A, src_align, dst_align, (int)cnt);          // tiled or register-rolling form (agt_pyr_rolling), workgroups per image: agt_pyr_blocks
        if (s == 0 && L >= 2) fused = plan_two_level(c, G, S, T, first, (int)cnt, src_align, dst_align, fused);
        S.pyr_nf[s] = (int)cnt;
        S.n_pyr[s] = agt_pyr_blocks(A) * B * (int)cnt;
        c->n_stage[s] += cnt;
        any = true;
    }
    return any;
}

// LK role: up to F of the frames whose pyramid is complete, behind frame G.lk_before.  Returns the frames tracked once the launch is through.
static long plan_lk(agt_ctx* c, const GroupEntry& G, AgtStepParams& S, AgtStepTables& T)
{
    const long f0 = G.lk_before;                 // the frame before the group
    long cnt = G.done_before[G.L] - f0;
    if (cnt <= 0) return c->n_lk;
    if (cnt > G.F) cnt = G.F;
    // level 0 geometry comes from the frame's own registration; a group needs it uniform
    const int pslot = ring_slot(c, f0);
    for (long k = 1; k <= cnt; k++) {
        const int q = ring_slot(c, f0 + k);
        if (!same_geometry(c->frame[q], c->frame[pslot])) { cnt = k > 1 ? k - 1 : 1; break; }
    }
    fill_tracker_lk(c, &S.lk, pslot, ring_slot(c, f0 + 1));
    fill_lk_table(c, T.lk, f0, (int)cnt);        // (arrival counters: attached by plan_pose)
    S.lk_nf = (int)cnt;
    S.n_lk = 1; S.lk_B = G.B;
    return c->n_lk += cnt;
}

// Pose role.  Frames it may take: everything tracked before this launch; chained, also the frames tracked BY it (lk_before + 1 ..
// lk_after), waiting for each one's counter -- all of them when nothing more is registered (a drain: the last frames' latency counts),
// all but the newest while frames keep coming (the role then never stalls: the LK role works one frame ahead of it)
static void plan_pose(agt_ctx* c, const GroupEntry& G, long lk_after, AgtStepParams& S, AgtStepTables& T)
{
    long avail = G.lk_before;
    if (G.fits) avail = lk_after - (lk_after < c->trk_frame && lk_after > G.lk_before ? 1 : 0);
    long cnt = avail - c->n_pnp;
    if (cnt <= 0) return;
    if (cnt > G.F) cnt = G.F;
    const long first = c->n_pnp + 1;
    const int slot = ring_slot(c, first);
    fill_estimate(c, &S.pnp, c->corners[slot], c->status[slot], c->frame[slot].state_out, nullptr);
    arm_host_seq(c, &S.pnp, first);
    for (long k = 0; k < cnt; k++) {
        const long f = first + k;
        const int q = ring_slot(c, f);
        T.pnp.img[k] = c->corners[q]; T.pnp.mask[k] = c->status[q]; T.pnp.so[k] = c->frame[q].state_out;
        if (f > G.lk_before) {
            // tracked by this launch (frame f - lk_before - 1 of its LK group): the LK role counts the frame's corners in (device-scope
            // stores + acknowledgement, only for the frames somebody waits for), the PnP wave waits for the count
            c->lk_target[q] += (unsigned)c->trk_n;
            T.lk.done[f - G.lk_before - 1] = c->lk_done + (size_t)q * c->cfg.max_streams;
            T.pnp.wait[k] = T.lk.done[f - G.lk_before - 1]; T.pnp.target[k] = c->lk_target[q];
        }
    }
    S.pnp_nf = (int)cnt;
    S.n_pnp = G.B;
    c->n_pnp += cnt;
}

// The fault-injection knobs of the diagnostic libraries, between plan and issue (the product: nothing).  Each counts, process-wide, the
// launches that satisfy ITS condition: tests/test_gpu_tracker.py addresses a launch by that count.
static void debug_inject(const AgtStepParams& S, AgtStepTables& T)
{
    // AGT_CHAIN_WITHHOLD=k makes the k-th launch with chained waits expect one arrival more than its LK role delivers for the SECOND
    // waited frame (the first if there is only one): the give-up path
    if (const long wh = AGT_KNOB("AGT_CHAIN_WITHHOLD", 0)) {
        static long seen = 0;
        int waited[2] = { -1, -1 }, nw = 0;
        for (int k = 0; k < S.pnp_nf && nw < 2; k++) if (T.pnp.wait[k]) waited[nw++] = k;
        if (wh > 0 && nw > 0 && ++seen == wh) T.pnp.target[waited[nw - 1]] += 1;
    }
    // AGT_TABLE_POISON_PNP=k / AGT_TABLE_POISON_LK=k put a word that cannot be an address (the bits of a NaN) into the second frame's
    // entry of the k-th launch whose pose / LK role runs more than one frame -- what a stale or clobbered LDS table would hand the
    // role: the launch must drain, flag and report, not fault
    const long pk = AGT_KNOB("AGT_TABLE_POISON_PNP", 0), lk = AGT_KNOB("AGT_TABLE_POISON_LK", 0);
    static long seen_p = 0, seen_l = 0;
    if (pk > 0 && S.pnp_nf > 1 && ++seen_p == pk) T.pnp.img[1] = (const float*)0x7ff8dead00000000ull;
    if (lk > 0 && S.lk_nf > 1 && ++seen_l == lk) T.lk.img[2][0] = (const uint8_t*)0x7ff8dead00000000ull;
}

static int issue_fused(agt_ctx* c, const AgtStepParams& S, const AgtStepTables& T)
{
    // a launch with pyramid work only (the first one of a run) goes out as the pyramid kernel proper: eight workgroups per
    // CU instead of the one the fused kernel's register budget leaves (16 frames of 720p: ~7 us instead of ~12)
    const int roles = (S.n_lk > 0 || S.n_pnp > 0) ? AGT_STEP_ALL : AGT_STEP_PYR;
    hipError_t e = agt_launch_step(c->stream, S, T, c->cfg.win, roles);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// ---- split mode (issue_split).  The pyramid and the pose role alike: `stream` waits for both halves of LK launch `lk_wait` (its event
// slot; -1 = none to wait for), the role's launch, its event `done`.
static int split_role(agt_ctx* c, const AgtStepParams& S, const AgtStepTables& T, int roles, hipStream_t stream, int lk_wait, hipEvent_t done)
{
    const SplitEvents& E = c->split;
    hipError_t e = hipSuccess;
    if (lk_wait >= 0) {
        e = hipStreamWaitEvent(stream, E.ev[SplitEvents::LK_DONE][lk_wait], 0);
        if (e == hipSuccess) e = hipStreamWaitEvent(stream, E.ev[SplitEvents::LK2_DONE][lk_wait], 0);
    }
    if (e == hipSuccess) e = agt_launch_step(stream, S, T, c->cfg.win, roles);
    if (e == hipSuccess) e = hipEventRecord(done, stream);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// One stand-alone LK launch per frame f0 + 1 .. f0 + nf (and half: streams [0, B1) on sL, [B1, B) on sL2), back to back on its stream
// (as a role with an in-kernel frame loop the one-wave-per-corner kernel needs 240 B of scratch per lane at its 128-register budget
// and runs at half speed)
static int split_lk_frames(agt_ctx* c, hipStream_t sL, hipStream_t sL2, long f0, int nf, int B, int B1)
{
    const bool two = B1 < B;
    for (int k = 1; k <= nf; k++) {
        const int ps = ring_slot(c, f0 + k - 1), sl = ring_slot(c, f0 + k);
        // (waves = 1: a half is sized by the whole batch's kernel choice, not by its own corner count)
        int rc = track_lk_on(c, sL, ps, sl, B1, 0, two ? 1 : 0);
        if (rc == AGT_OK && two) rc = track_lk_on(c, sL2, ps, sl, B - B1, B1, 1);
        if (rc) return rc;
    }
    return AGT_OK;
}

// The LK role of the group; p_before: event slot of the pyramid launch BEFORE this group's (-1 = none since the last join)
static int split_lk(agt_ctx* c, const GroupEntry& G, const AgtStepParams& S, const AgtStepTables& T, int p_before)
{
    SplitEvents& E = c->split;
    const int B = G.B, slot = E.next_slot(SplitEvents::LK);
    hipStream_t sL = c->ms_stream[1], sL2 = c->ms_stream[0];
    // The per-frame LK launches of a group depend on each other (a corner starts where it ended), leave ~4 us between one
    // kernel's end and the next one's start on their stream, and each lasts as long as its slowest corner.  A batch of the
    // one-wave-per-corner kernel whose halves still hold >= 512 corners goes out as two launches per frame on two streams,
    // streams [0, B1) and [B1, B), both with the one-wave kernel: each half's gaps and tails are filled by the other half's
    // kernel.  Every wait on / record of the LK role is done for both streams.  (Round 3: the halves used to be taken
    // only from 44 streams of 48 corners on; 22 .. 43 streams gain 12-20 % -- 42 streams 43.9 -> 36.6 us per step.  Four
    // quarters on four streams lose badly -- 64 streams 160 us, 86 with GPU_MAX_HW_QUEUES=8 against 49.7: more streams than
    // hardware queues, and four kernels of <= 1 wave per SIMD each stretch one another.)
    // Up to 1024 corners in flight (the four-waves-per-corner body): the LK role of the WHOLE group as one launch --
    // lk_group_kernel, the frame-chained body of the fused step with its own register budget (153 VGPRs, three workgroups
    // per CU) -- instead of one ~17 us launch + ~5 us gap per frame (round 3: 16 streams 33.9 -> see profiles/r03_stream_sweep.txt).
    const bool lk_group = agt_lk_wide(c->trk_n, B);
    const int B1 = (!lk_group && (long)c->trk_n * (B / 2) >= 512) ? B / 2 : B;
    const bool two = B1 < B;
    hipError_t e = hipSuccess;
    hipEvent_t first = nullptr;
    if (p_before >= 0) first = E.ev[SplitEvents::PYR_DONE][p_before];
    else {
        // no pyramid launch since the last join (single-level pyramids, or the first LK of a run): order the LK streams
        // behind the caller's stream explicitly (reset's corner copy, earlier modes' pyramids)
        first = E.ev[SplitEvents::MISC][SplitEvents::HANDOVER];
        e = hipEventRecord(first, c->stream);
    }
    for (int h = 0; h < (two ? 2 : 1) && e == hipSuccess; h++) {
        hipStream_t sh = h ? sL2 : sL;
        e = hipStreamWaitEvent(sh, first, 0);
        if (e == hipSuccess && E.pose_hist[1] >= 0) e = hipStreamWaitEvent(sh, E.ev[SplitEvents::POSE_DONE][E.pose_hist[1]], 0);
    }
    if (e == hipSuccess && lk_group) e = agt_launch_step(sL, S, T, c->cfg.win, AGT_STEP_LK);
    if (e != hipSuccess) return hip_fail(c, e);
    if (!lk_group) {
        int rc = split_lk_frames(c, sL, sL2, G.lk_before, S.lk_nf, B, B1);
        if (rc) return rc;
    }
    e = hipEventRecord(E.ev[SplitEvents::LK_DONE][slot], sL);
    // (recorded on the second stream in any case: an idle stream's event is complete at once, the waits stay uniform)
    if (e == hipSuccess) e = hipEventRecord(E.ev[SplitEvents::LK2_DONE][slot], two ? sL2 : sL);
    if (e != hipSuccess) return hip_fail(c, e);
    E.pushed_lk(slot);
    c->ms_active = 1;
    return AGT_OK;
}

// The same group as three launches, one per role, each with its own LDS size and register budget:
// pyramid on the caller's stream (the frames come from there), LK and PnP on two library streams.  The roles of one
// group are independent (the pipeline skews them across frames), so the three launches overlap; ordering is by events:
//   LK(k)  waits for pyramid(k-1)   (its images)          and for PnP(k-2)  (ring reuse of corner / status entries)
//   PnP(k) waits for LK(k-1)        (its corners)
//   pyramid(k) waits for LK(k-3)    (ring reuse of level entries: split mode keeps AGT_SPLIT_SLACK = 2 groups of extra
//                                    ring entries, so the HBM-bound pyramid launches run AHEAD of the LK launches they share
//                                    the chip with and never sit on the critical path; the wait also keeps the caller's
//                                    stream behind the readers of frames handed over (L + 6) groups ago, so stream-ordered
//                                    allocators may recycle those)
// Ten HIP calls per GROUP of F frames (round 1 issued thirteen per frame).
// A role's n-th launch records event slot n % AGT_EV_SLOTS, so the slot a wait names (at most three launches of its role old) is not
// re-recorded before it.  (The slots used to follow the group count: a role that sat groups out could wait on a slot that a NEWER
// launch of the same role and stream had re-recorded -- later completion, so that could only over-synchronise.)
static int issue_split(agt_ctx* c, const GroupEntry& G, const AgtStepParams& S, const AgtStepTables& T)
{
    int rc = ms_init(c);
    if (rc) return rc;
    SplitEvents& E = c->split;
    // the roles of this group wait for the launches of the groups BEFORE it: read before this group's launches enter the histories
    const int p_before = E.last_pyr, l_before = E.lk_hist[0];
    bool p_work = false;
    for (int s = 0; s < AGT_MAX_LEVELS - 1; s++) p_work |= S.n_pyr[s] > 0;
    if (p_work) {
        const int slot = E.next_slot(SplitEvents::PYR);
        rc = split_role(c, S, T, AGT_STEP_PYR, c->stream, E.lk_hist[AGT_SPLIT_SLACK], E.ev[SplitEvents::PYR_DONE][slot]);
        if (rc) return rc;
        E.pushed_pyr(slot);
    }
    if (S.n_lk > 0) {
        rc = split_lk(c, G, S, T, p_before);
        if (rc) return rc;
    }
    if (S.n_pnp > 0) {
        const int slot = E.next_slot(SplitEvents::POSE);
        rc = split_role(c, S, T, AGT_STEP_PNP, c->ms_stream[2], l_before, E.ev[SplitEvents::POSE_DONE][slot]);
        if (rc) return rc;
        E.pushed_pose(slot);
        c->ms_active = 1;
    }
    return AGT_OK;
}

// fmax: the most frames a stage advances by in this call (0 = c->group).  The split pipeline (big batches: three launches per group)
// runs groups of c->group frames in the steady state but SMALLER ones while it fills and drains (round 6, tools/trace_blocks.py: of a
// 256-frame block of 64 streams 8 % was the first pyramid launch with nothing beside it and the last pose launch with nothing beside it --
// a stage's launch covers a whole group, and the next stage waits for all of it): split_ramp() frames at first, doubling per launch.
static int split_ramp(const agt_ctx* c) { const int r = c->group / 4; return r < 2 ? (c->group < 2 ? c->group : 2) : r; }
static int launch_group(agt_ctx* c, int B, int fmax = 0)
{
    GroupEntry G;
    G.L = c->eff_max_level; G.F = (fmax > 0 && fmax < c->group) ? fmax : c->group; G.B = B;
    G.fits = agt_step_fits(c->trk_n, B);
    G.done_before[0] = c->trk_frame;
    for (int s = 0; s < G.L; s++) G.done_before[s + 1] = c->n_stage[s];
    G.lk_before = c->n_lk;
    G.pyr_only = c->n_lk >= G.done_before[G.L] && c->n_pnp >= c->n_lk;
    AgtStepParams S; AgtStepTables T;
    memset(&S, 0, sizeof(S)); memset(&T, 0, sizeof(T));
    S.pnp.fault = c->fault_dev;                  // (also where the launch has no pose role: the LK role reports a table it cannot use through it)
    const bool pyr_work = plan_pyramid(c, G, S, T);
    const long lk_after = plan_lk(c, G, S, T);
    plan_pose(c, G, lk_after, S, T);
    if (!pyr_work && S.n_lk == 0 && S.n_pnp == 0) return AGT_OK;
    debug_inject(S, T);
    return G.fits ? issue_fused(c, S, T) : issue_split(c, G, S, T);
}

// The part of registering frame T+1 that comes before the registration itself: ring modulus of the mode (fits: agt_step_fits of the
// batch, the fused form; otherwise the split one), a free ring entry.
static int pipelined_entry(agt_ctx* c, int B, bool fits)
{
    c->prebuilt_t = -1;
    // ring modulus of this mode: (L + 2) groups, plus the split mode's slack when the entries are available
    int groups = c->eff_max_level + 2 + (fits ? 0 : AGT_SPLIT_SLACK);
    if (groups * c->group > AGT_RING_MAX) groups = c->eff_max_level + 2;
    const int want = groups * c->group > AGT_SLOTS ? groups * c->group : AGT_SLOTS;
    if (want != c->live_ring) {
        int rc = join_pipeline(c);            // only the newest frame is live afterwards
        if (rc) return rc;
        rc = ensure_ring(c, want);
        if (rc) return rc;
        ring_move(c, c->trk_frame, c->live_ring, want);
        c->live_ring = want;
    }
    // The ring entry frame t takes must be free: its previous tenant, frame t - M, has to be past its pose solve and past the
    // LK of the frame after it (which reads it as the previous image).  The ring size follows from every stage advancing F
    // frames per launch; groups cut short (frames of differing pitch) let stages fall behind that rhythm.
    const long t = c->trk_frame + 1, M = c->live_ring;
    while (c->n_pnp < t - M || c->n_lk < t - M + 1) {
        const long before = c->n_pnp + c->n_lk + c->n_stage[0];
        int rc = launch_group(c, B);
        if (rc) return rc;
        if (c->n_pnp + c->n_lk + c->n_stage[0] == before) return AGT_ERR_STATE;      // (cannot happen: work was pending)
    }
    return AGT_OK;
}

// Register frame T+1 of the fused pipeline; a launch goes out once `group` frames wait for their first stage.
int step_pipelined(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B, double* d_state_out)
{
    const bool fits = agt_step_fits(c->trk_n, B);
    int rc = pipelined_entry(c, B, fits);
    if (rc) return rc;
    const long t = c->trk_frame + 1;
    register_frame(c, ring_slot(c, t), d_frames, pitch, batch_stride, B, d_state_out);
    c->trk_frame = t;
    const long first_done = c->eff_max_level > 0 ? c->n_stage[0] : c->n_lk;
    if (fits) {
        if (t - first_done < c->group) return AGT_OK;
        return launch_group(c, B);
    }
    // split pipeline: groups grow from split_ramp() to c->group frames while the pipeline fills (see launch_group)
    if (c->ramp <= 0 || c->ramp > c->group) c->ramp = split_ramp(c);
    if (t - first_done < c->ramp) return AGT_OK;
    rc = launch_group(c, B, c->ramp);
    c->ramp = c->ramp * 2 > c->group ? c->group : c->ramp * 2;
    return rc;
}

// Frame T+1 of ONE stream arrives in pinned HOST memory (h_dev: its device address): upload and pyramid in one launch -- the
// two-level register-rolling pass reads the frame over PCIe, stores its level 0 to d_gray and levels 1 / 2 to the frame's ring
// entry (agt_pyramid.hip agt_launch_pyr_upload2) -- and the frame is registered with its pyramid stages done; the LK | PnP launch
// follows at the join as ever.  Returns 1 when the form does not apply (geometry, pyramid work of earlier frames still pending):
// nothing has been enqueued for the frame then and the caller copies and calls agt_track_frame.  (The caller has checked agt_step_fits.)
int step_pipelined_uploaded(agt_ctx* c, const uint8_t* h_dev, uint8_t* d_gray, size_t gpitch, double* d_state_out)
{
    if (c->eff_max_level != 2 || c->trk_B != 1) return 1;
    int rc = pipelined_entry(c, 1, true);
    if (rc) return rc;
    const long t = c->trk_frame + 1;
    if (c->n_stage[0] != t - 1 || c->n_stage[1] != t - 1) return 1;
    const int slot = ring_slot(c, t);
    const int W = c->cfg.width, H = c->cfg.height;
    hipError_t e = agt_launch_pyr_upload2(c->stream, h_dev, W, H, (long)W, d_gray, (long)gpitch, c->lmem[slot][1], c->lpitch[1], c->lmem[slot][2], c->lpitch[2]);
    if (e == hipErrorInvalidValue) { (void)hipGetLastError(); return 1; }
    if (e != hipSuccess) return hip_fail(c, e);
    register_frame(c, slot, d_gray, gpitch, gpitch * (size_t)H, 1, d_state_out);
    c->trk_frame = t;
    c->n_stage[0] = c->n_stage[1] = t;
    return AGT_OK;
}

// Drain the software pipeline: enqueue the remaining stages of every frame supplied so far.
// (Enqueue only; the results are ordered on the context's stream like any other work.)
int join_pipeline(agt_ctx* c)
{
    if (c->trk_ready != 2) return AGT_OK;
    // (split pipeline: the drain runs in groups of split_ramp() frames -- the last pose launch then trails the last LK launch by a
    // quarter of a group instead of a whole one; afterwards the pipeline is empty and fills again in small groups)
    const int fmax = agt_step_fits(c->trk_n, c->trk_B) ? 0 : split_ramp(c);
    while (c->n_pnp < c->trk_frame) {
        int rc = launch_group(c, c->trk_B, fmax);
        if (rc) return rc;
    }
    c->ramp = 0;
    return c->ms_active ? ms_join(c) : AGT_OK;
}

// move frame `f`'s ring entry when the ring size changes (only the newest frame is live after a join)
void ring_move(agt_ctx* c, long f, int old_ring, int new_ring)
{
    const int a = (int)(f % old_ring), b = (int)(f % new_ring);
    if (a == b) return;
    for (int l = 1; l < AGT_MAX_LEVELS; l++) { uint8_t* t = c->lmem[a][l]; c->lmem[a][l] = c->lmem[b][l]; c->lmem[b][l] = t; }
    { float* t = c->corners[a]; c->corners[a] = c->corners[b]; c->corners[b] = t; }
    { uint8_t* t = c->status[a]; c->status[a] = c->status[b]; c->status[b] = t; }
    c->frame[b] = c->frame[a]; c->frame[a].B = 0;
}

// ---- (3) the serial step
// next_frame != null (clip submission with the dense stage): the caller will hand that frame in next, with the same pitch and
// stream stride -- its two-level pyramid pass rides in one of this frame's launches (the chained LK | PnP launch, the four-wave PnP
// launch, or the second dense launch) instead of being the first launch of its own chain, and this frame's last dense step is left
// to that frame's LK launch (c->dense_pending).

// agt_tracker_fb_check: the verdict launch behind the tracker's LK launch prev_slot -> slot.  A dropped corner is a corner LK lost in
// this frame: status 0 from here on (sticky), the forward position kept in its entry and carried.
// Under agt_tracker_predict the backward pass starts at arrival - flow (one more small launch writes those points): started at the
// arrival it would fail for the reason the unseeded forward pass does.
static int track_fb_on(agt_ctx* c, hipStream_t stream, int prev_slot, int slot, int B)
{
    const float* back = nullptr;
    if (c->opt.pred_px > 0.0) {
        const AgtFlowBackParams q = { c->trk_n, c->corners[slot], c->pred_flow, c->pred_back };
        hipError_t e = agt_launch_flow_back(stream, q, B);
        if (e != hipSuccess) return hip_fail(c, e);
        back = c->pred_back;
    }
    return lk_verdict_on(c, stream, prev_slot, slot, c->corners[prev_slot], c->corners[slot], c->status[slot], nullptr, nullptr, c->trk_n, B,
                         AGT_TERM_COUNT | AGT_TERM_EPS, c->lk_max_count, c->lk_eps, 0, c->lk_min_eig, c->opt.fb_max_px, back);
}

// The launch form of one serial frame, decided (serial_form) before anything of it is issued.
struct SerialForm {
    bool lk_role_launch;         // LK as the LK role of the step, a one-frame group, instead of the stand-alone LK launch
    bool ride;                   // the next frame's two-level pyramid pass rides in one of this frame's launches: ...
    bool chain_pnp;              // ... LK and PnP of the frame in ONE launch, which then carries the ride as well
    bool ride_pnp;               // ... the ride in the PnP launch (otherwise, and unchained: in the dense stage's second launch)
    bool defer;                  // the dense stage's last step is left to the NEXT frame's LK launch
};

// dense: the frame runs the dense stage; spans: stage spans are being recorded (agt_profile_begin)
// (the frame is registered in ring entry `slot`, the one before it in pslot, the next one would go to nslot)
static SerialForm serial_form(const agt_ctx* c, int pslot, int slot, int nslot, int B, bool dense, bool spans, const uint8_t* next_frame)
{
    SerialForm f;
    const bool dense_iters = dense && c->dn_iters > 0;
    // four waves per corner: the LK role of the step as a one-frame group (the frame-chained body; see agt_step.hip lk_role)
    const bool wide = c->cfg.win == 21 && agt_lk_wide(c->trk_n, B);
    // (an option that needs the stand-alone LK launch: not the LK role, not the chained or the deferring forms that build on it)
    const bool own_lk = c->opt.needs_lk_launch();
    f.lk_role_launch = wide && !own_lk && same_geometry(c->frame[pslot], c->frame[slot]);
    // Clip submission: the next frame's two-level pyramid pass rides in one of this frame's launches -- the PnP launch where that
    // is the four-wave kernel (n > 64: one workgroup per stream, the chip idles beside it), else the dense stage's second launch.
    // (Measured on configs[4], us per frame: no ride 89.0; in the PnP launch 84.0-84.5; in the dense launch 84.0-85.3; in the LK
    // launch 84.5-84.8 as tiles behind the LK role launch's own workgroups, 86.5 as the pyramid role of the fused step kernel.)
    f.ride = next_frame && c->eff_max_level == 2 && B <= AGT_PYR2_MAX_B && nslot != slot && nslot < c->ring &&
             ((uintptr_t)next_frame & 3) == 0 && (agt_pnp_can_ride(c->trk_n) || dense_iters);
    // Dense clips with the cooperative solver (64 < n <= 256): LK and PnP of the frame in ONE launch, the solver waiting for the
    // frame's arrival count (agt_step.hip lk_pnp_coop_kernel); the next frame's pyramid pass then rides in that launch as well
    // (while trackers + solvers are co-resident at the one workgroup per CU the solver's registers leave: more streams keep the LK
    // launch of its own, whose 78 registers put several workgroups on a CU)
    // (the LK role's grid is rounded up to a multiple of 8; the device's CU count, not a literal: ADVICE r4)
    f.chain_pnp = f.lk_role_launch && dense_iters && !spans && agt_pnp_can_ride(c->trk_n) &&
                  (long)agt_xcd_grid((long)c->trk_n * B, 3) + B <= c->chip.cus;
    f.ride_pnp = f.ride && agt_pnp_can_ride(c->trk_n) && !f.chain_pnp;
    // Clip submission: the stage's last step (final update + re-seed, a one-workgroup launch of 5.5 us) is left to the NEXT
    // frame's LK launch, whose workgroups do it as their prologue (agt_step.hip lk_reseed_kernel) -- when that launch will be the
    // four-waves-per-corner LK role launch (same geometry as this frame's) and no stage spans are being recorded
    f.defer = next_frame && !spans && dense_iters && wide && !own_lk;
    return f;
}

// LK of frame t as the one-frame LK role launch; chained, the pose solve `p` in the same launch.  Unlike launch_group, whose plans
// advance the context's counters while they fill the tables, the arrival target (lk_target) and dense_pending change here only once
// the launch is known to be out: this form has an error path (agt_track_frames_dense), and a failed launch must leave the counters'
// bookkeeping and the deferred dense step as they were.
static int serial_lk_role(agt_ctx* c, const SerialForm& f, const AgtPnpParams& p, long t, int B, const AgtPyrArgs* npyr)
{
    const int slot = ring_slot(c, t);
    AgtStepParams S; AgtStepTables T;
    memset(&S, 0, sizeof(S)); memset(&T, 0, sizeof(T));
    fill_tracker_lk(c, &S.lk, ring_slot(c, t - 1), slot);
    fill_lk_table(c, T.lk, t - 1, 1);
    S.lk_nf = 1; S.n_lk = 1; S.lk_B = B;
    if (f.chain_pnp) {
        S.pnp = p; S.pnp_nf = 1; S.n_pnp = B;
        T.lk.done[0] = c->lk_done + (size_t)slot * c->cfg.max_streams;
        T.pnp.img[0] = c->corners[slot]; T.pnp.mask[0] = c->status[slot]; T.pnp.so[0] = p.state_out;
        T.pnp.wait[0] = T.lk.done[0]; T.pnp.target[0] = c->lk_target[slot] + (unsigned)c->trk_n;
        // knobs: AGT_CHAIN_WITHHOLD_DENSE=k makes the k-th chained LK | PnP launch of the dense tracker expect one arrival more than
        // its LK role delivers (tests/test_dense.py drives the solver's give-up path with it)
        { const long wh = AGT_KNOB("AGT_CHAIN_WITHHOLD_DENSE", 0); static long seen = 0; if (wh > 0 && ++seen == wh) T.pnp.target[0] += 1; }
    }
    hipError_t e;
    if (c->dense_pending || f.chain_pnp) {
        e = agt_launch_lk_reseed(c->stream, S, T, c->cfg.win, c->dense_pending ? &c->dense_final : nullptr, (f.ride && f.chain_pnp) ? npyr : nullptr);
        if (e == hipSuccess) {                  // on failure dense_pending stays set: the caller's error path flushes it (agt_launch_dense_final)
            c->dense_pending = 0;
            if (f.chain_pnp) c->lk_target[slot] += (unsigned)c->trk_n;
        }
    } else e = agt_launch_step(c->stream, S, T, c->cfg.win, AGT_STEP_LK);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// dense photometric + geometric refinement of the frame's accepted pose, then (reseed) the corner set from it
static int serial_dense(agt_ctx* c, const SerialForm& f, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int slot, int B,
                        double* d_dense_out, hipEvent_t* pev, const AgtPyrArgs* npyr)
{
    agt_dense::DenseParams P = dense_params_on(c);
    P.img = d_frames; P.pitch = (long)pitch; P.ibatch = (long)batch_stride; P.w = c->cfg.width; P.h = c->cfg.height;
    P.mxyz = c->dn_xyz; P.mt = c->dn_t; P.M = c->dn_M; P.obj = c->obj; P.ipts = c->corners[slot]; P.mask = c->status[slot]; P.N = c->trk_n;
    P.cam = c->cam; P.pose = c->pose; P.photo_weight = c->dn_weight; P.rec = d_dense_out;
    if (c->dn_reseed) { P.seed_pts = c->corners[slot]; P.seed_status = c->status[slot]; }
    hipError_t e = agt_launch_dense(c->stream, P, B, c->dn_iters, pev ? pev + 4 : nullptr, 2 * AGT_PROF_DENSE_MAX,
                                    (f.ride && !f.ride_pnp && !f.chain_pnp) ? npyr : nullptr, f.defer ? &c->dense_final : nullptr);
    if (e == hipSuccess && f.defer) c->dense_pending = 1;
    if (pev) c->prof_dense[c->prof_n - 1] = c->dn_iters < AGT_PROF_DENSE_MAX ? c->dn_iters : AGT_PROF_DENSE_MAX;
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

int step_serial(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B,
                double* d_state_out, double* d_dense_out, hipEvent_t* pev, const uint8_t* next_frame)
{
    int rc = join_pipeline(c);            // a mode switch drains the pipeline first
    if (rc) return rc;
    const long t = c->trk_frame + 1;
    const int slot = ring_slot(c, t), pslot = ring_slot(c, t - 1), nslot = ring_slot(c, t + 1);
    hipStream_t M = c->stream;
    if (pev) (void)hipEventRecord(pev[0], M);
    const RingFrame now = { d_frames, (long)pitch, (long)batch_stride, B, nullptr }, &held = c->frame[slot];
    const bool prebuilt = c->prebuilt_t == t && held.ptr == now.ptr && same_geometry(held, now) && held.B == now.B;
    c->prebuilt_t = -1;
    rc = prebuilt ? AGT_OK : pyramid_build_on(c, M, slot, d_frames, pitch, batch_stride, B);
    if (rc) return rc;
    if (pev) (void)hipEventRecord(pev[1], M);
    const SerialForm f = serial_form(c, pslot, slot, nslot, B, d_dense_out != nullptr, pev != nullptr, next_frame);
    AgtPyrArgs npyr[2];
    if (f.ride) {
        // frame t + 1 in its ring entry, as pyramid_build_on would leave it (the serial step reads no state_out from the ring)
        register_frame(c, nslot, next_frame, pitch, batch_stride, B, nullptr);
        AgtLevel lv[AGT_MAX_LEVELS];
        fill_levels(c, nslot, lv);
        agt_pyr2_args(lv, B, npyr);
        c->prebuilt_t = t + 1;
    }
    AgtPnpParams p;
    fill_estimate(c, &p, c->corners[slot], c->status[slot], d_state_out, c->corners[slot], c->status[slot]);
    arm_host_seq(c, &p, t);
    if (d_dense_out) {
        rc = dense_scratch(c, agt_dense_doubles(c->dn_M, B), B);
        if (rc) return rc;
        p.dense_pose = c->pose; p.dense_done = c->dense_done; p.dense_rec = d_dense_out;
    }
    if (f.lk_role_launch) rc = serial_lk_role(c, f, p, t, B, npyr);
    else {
        if (c->dense_pending) {          // (cannot happen: the deferral is decided with this frame's launch form known)
            c->dense_pending = 0;
            hipError_t e = agt_launch_dense_final(M, c->dense_final, B);
            if (e != hipSuccess) return hip_fail(c, e);
        }
        const bool pred = c->opt.pred_px > 0.0;
        if (pred && (rc = track_seed_on(c, M, pslot, slot, B))) return rc;
        rc = track_lk_on(c, M, pslot, slot, B, 0, 0, pred ? AGT_LK_USE_INITIAL_FLOW : 0);
        if (rc == AGT_OK && c->opt.fb_max_px > 0.0) rc = track_fb_on(c, M, pslot, slot, B);
    }
    if (rc) return rc;
    if (pev) (void)hipEventRecord(pev[2], M);
    if (!f.chain_pnp && (rc = pose_step_on(c, M, &p, B, pslot, f.ride_pnp ? npyr : nullptr))) return rc;      // (chained: the pose solve is out with the LK role)
    if (pev) { (void)hipEventRecord(pev[3], M); c->prof_n++; }
    if (d_dense_out) rc = serial_dense(c, f, d_frames, pitch, batch_stride, slot, B, d_dense_out, pev, npyr);
    if (rc) return rc;
    frame_complete(c, t);
    return AGT_OK;
}
