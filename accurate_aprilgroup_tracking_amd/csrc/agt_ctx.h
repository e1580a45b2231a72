// agt_ctx.h -- the context of the C ABI and the host internals its sources share (agt_api.hip: context lifecycle and the device
// table; agt_api_calls.hip: the stateless calls; agt_api_tracker.hip: the tracker's entry points; agt_api_live.hip: the live camera
// loop; agt_api_undistort.hip: undistortion; agt_tracker_frames.hip: what a tracked frame is issued with and its launch forms, whose
// own declarations are in agt_tracker.h).
// The entry points take their C linkage from include/agt_hip.h; nothing declared here leaves the library (agt_hip.map).
#pragma once
#include "agt_kernels.h"
#include "agt_knobs.h"
#include <time.h>

#define AGT_SLOTS 4              // ring entries every context owns (slots 0 / 1 are also the public pyramid slots)
#define AGT_RING_MAX 224         // (levels + 1) * AGT_MAX_GROUP frames in flight at the deepest pipeline
#define AGT_EV_SLOTS 8           // events of the split pipeline, per kind: a launch waits for events at most three launches of their role old (SplitEvents::lk_hist), slots are re-recorded modulo 8
// The two-level pyramid pass saves a launch / pipeline stage and 16 % of the pyramid's HBM bytes, but its 41 KB workgroups
// (3 per CU, eight barriers per tile) stream at 2.5 TB/s against 3.9 + 3.4 TB/s for two single-level passes (8 per CU): it is
// used where the stage count matters (few streams), the two passes where throughput does (measured at 64 x 720p: 30.5 vs 25 us).
#define AGT_PYR2_MAX_B 8
#define AGT_TILT_SLOTS 8          // device table of tilted-sensor matrices: slot 0 the tracker's camera, 1.. the stateless calls'
#define AGT_SPLIT_SLACK 2        // split mode: groups of extra ring entries (pyramid launches run that far ahead of LK)

// Event state of the split pipeline (agt_tracker_frames.hip issue_split).  A role's n-th launch records slot n % AGT_EV_SLOTS of its row, and
// the histories name the slots of its most recent launches: the events later launches of the OTHER roles wait for (-1 = none: nothing
// of that role is in flight).  Plain data: valid when zero-filled except for the histories, which reset_history() sets.
struct SplitEvents {
    enum Role { PYR, LK, POSE };
    enum Row { PYR_DONE, LK_DONE, MISC, POSE_DONE, LK2_DONE, ROWS };        // LK2_DONE: the second half of the streams (ms_stream[0])
    enum Misc { JOIN_LK, JOIN_POSE, HANDOVER, JOIN_LK2 };                   // slots of row MISC: the joins of the three library streams, the caller's stream handing over to LK
    hipEvent_t ev[ROWS][AGT_EV_SLOTS];
    long n[3];                               // launches issued in split mode per Role
    int last_pyr;                            // event slot of the most recent pyramid launch
    int lk_hist[3];                          // event slots of the three most recent LK launches, newest first
    int pose_hist[2];                        // event slots of the two most recent PnP launches, newest first
    int next_slot(Role r) const { return (int)(n[r] % AGT_EV_SLOTS); }
    void reset_history() { last_pyr = -1; lk_hist[0] = lk_hist[1] = lk_hist[2] = -1; pose_hist[0] = pose_hist[1] = -1; }
    void pushed_pyr(int slot) { last_pyr = slot; n[PYR]++; }
    void pushed_lk(int slot) { lk_hist[2] = lk_hist[1]; lk_hist[1] = lk_hist[0]; lk_hist[0] = slot; n[LK]++; }
    void pushed_pose(int slot) { pose_hist[1] = pose_hist[0]; pose_hist[0] = slot; n[POSE]++; }
};

// What a ring entry knows about the frame it holds: level 0 is the caller's buffer (B streams of it; 0 = no pyramid built), levels >= 1
// are the entry's own (agt_ctx::lmem).  state_out: where the frame's record goes -- meaningful only for frames the pipelined form
// registered (agt_tracker_frames.hip), moved along with the entry, read by that form's pose role alone.
struct RingFrame { const uint8_t* ptr; long pitch, bstride; int B; double* state_out; };
// frames of one group launch / of a chained pair share pitch and stream stride of level 0
inline bool same_geometry(const RingFrame& a, const RingFrame& b) { return a.pitch == b.pitch && a.bstride == b.bstride; }

// The tracker's options (agt_tracker_options, _tag_gate, _fb_check, _visibility, _consensus, _predict; enhance_ape: agt_tracker_reset)
// and the rules that follow from them -- THE place that says which option forces which launch form, and why:
//   fb_check   the backward pass is a launch of its own behind the stand-alone LK launch;
//   consensus  the hypothesis and vote launches sit between the LK and the pose launch;
//   predict    the seeds are an initial flow, which the chain body of the LK role does not take;
//     -> needs_lk_launch(): the frame's LK is the stand-alone launch -- not the LK role of the step, nor the chained or deferring
//        forms of the serial step that build on it (agt_tracker_frames.hip serial_form);
//   reproject  the refresh of a frame's corners comes out of its pose solve and feeds the next frame's LK, which the pipelined
//              forms run before that solve;
//     -> stage_by_stage(): with any of the four on, frames take the serial step whatever the pipeline depth.
//   visibility acts inside the reproject refresh only and changes no form.
// The dense forms (agt_track_frame(s)_dense) carry none of fb_check, visibility, consensus, predict: dense_refusal().
// Plain data, valid when zero-filled (everything off) but for min_points / gate_px, which agt_create sets.
struct TrackOptions {
    int reproject, min_points, tag_gate, enhance_ape;
    double gate_px, fb_max_px;               // fb_max_px: forward-backward threshold of the tracker's LK, px (0 = off)
    double vis_deg, vis_cos_max; int vis_cpt, vis_facing;      // the reproject refresh revives visible tags only (vis_deg = 0: off)
    double cons_px; int cons_cpt, cons_min;  // per-frame tag consensus in front of the pose step (cons_px = 0: off)
    double pred_px;                          // motion-predicted initial flow of the LK step (0 = off; its buffers: agt_ctx::pred_*)
    bool needs_lk_launch() const { return fb_max_px > 0.0 || cons_px > 0.0 || pred_px > 0.0; }
    bool stage_by_stage() const { return reproject || needs_lk_launch(); }
    // the dense stage's launch forms carry no backward pass, its re-seed no visibility rule, they leave no room for the consensus
    // launches and their LK role takes no initial flow
    int dense_refusal() const { return (fb_max_px > 0.0 || vis_deg > 0.0 || cons_px > 0.0 || pred_px > 0.0) ? AGT_ERR_UNSUPPORTED : AGT_OK; }
    // Whole tags: n corners are corners 4t .. 4t + 3 under the tag gate, whole tags under the visibility rule, whole tags and at most
    // 64 of them under consensus.  The codes differ by option (ABI).  agt_tracker_reset asks for its n; a setter asks for the options
    // as they would be with the tracker's n -- the options in force always fit it, so only the new value can object.
    int fits_corners(int n) const
    {
        if (tag_gate && n % tag_gate) return AGT_ERR_NPOINTS;
        return ((vis_deg > 0.0 && n % vis_cpt) || (cons_px > 0.0 && (n % cons_cpt || n / cons_cpt > 64))) ? AGT_ERR_ARG : AGT_OK;
    }
};

struct agt_ctx {
    agt_config cfg;
    AgtChip chip;                            // the device the context was created on (CU / XCD counts: launch rules and block orders)
    int lk_cap_cu;                           // agt_lk_occupancy_cu: resident one-wave LK workgroups per CU (0 = no cap, -1 = the library's choice)
    hipStream_t stream;
    int last_hip;
    int eff_max_level;                       // after OpenCV's early stop
    int lw[AGT_MAX_LEVELS], lh[AGT_MAX_LEVELS];
    long lpitch[AGT_MAX_LEVELS];             // levels >= 1 (context-owned)
    char* hcall_host; char* hcall_dev; unsigned long long hcall_n;      // host-mapped staging of the synchronous host-array calls (agt_solve_pnp_host)
    double* d_tilt; double tilt_host[AGT_TILT_SLOTS][18]; int tilt_valid[AGT_TILT_SLOTS]; int tilt_next;   // tilted-sensor matrices (camera_on)
    uint8_t* lmem[AGT_RING_MAX][AGT_MAX_LEVELS];
    RingFrame frame[AGT_RING_MAX];           // the frame each entry holds
    // tracker: rings (frame t lives in entry t % ring) so that one fused launch can work on pyramid
    // stage s of frames t-sF.., LK of frames t-LF.. and PnP of frames t-(L+1)F.. at once (F = group)
    int ring;                                // allocated ring entries: >= (L + 2) * group
    float* corners[AGT_RING_MAX];            // [B][n][2]
    uint8_t* status[AGT_RING_MAX];           // [B][n]
    int pipeline;                            // 1 = software-pipelined fused step (agt_step.hip)
    int group;                               // frames per fused launch (1..AGT_MAX_GROUP)
    int ramp;                                // split pipeline: frames per group while the pipeline fills (launch_group: split_ramp)
    int live_ring;                           // ring modulus in use (<= ring): (L + 2) * group, at least AGT_SLOTS
    // big batches: the three stages of a step run on three library-owned streams (stage kernels of different frames
    // overlap: 57 us against 93 us back to back at 64 streams); events carry the exact dependencies
    hipStream_t ms_stream[3];                // [1] LK, [0] LK of the second half of the streams, [2] PnP (the pyramid role runs on the caller's stream)
    int ms_pool_slot;                        // which set of the process's library streams the context holds (-1: none)
    int ms_ready, ms_active;                 // streams / events exist; frames are in flight on them
    // split mode (more corners in flight than the fused launch takes): the pipeline's groups go out as three launches,
    // pyramid on the caller's stream, LK and PnP on library streams (ms_stream[1], [2])
    SplitEvents split;
    long trk_frame;                          // frames supplied since reset (0 = only the reset frame)
    long prebuilt_t = -1;                    // serial step, clip submission: frame whose pyramid the previous frame's dense launch built (-1 = none)
    // clip submission of the dense stage: the previous frame's last step (final update + re-seed) waits for this frame's LK launch
    // (agt_step.hip lk_reseed_kernel); only ever set between two frames of one agt_track_frames_dense call
    int dense_pending = 0;
    AgtDenseFinal dense_final;
    long n_stage[AGT_MAX_LEVELS];            // frames whose pyramid stage s (level s -> s+1) is done
    long n_lk, n_pnp;                        // frames whose LK / PnP is done (enqueued)
    // chained launches (fused step): per ring entry, [max_streams] arrival counters the LK role counts corners into and
    // the PnP role of the same launch waits on; lk_target = the value the entry's counters reach once every corner
    // of its current frame is written (counters only ever grow: no reset, no reuse hazard)
    unsigned* lk_done;
    unsigned lk_target[AGT_RING_MAX];
    float* lkerr;                            // [B][n]
    float* obj;                              // [n][3]
    double* pose;                            // [B][6]
    AgtTrackState* tstate;                   // [B]
    AgtCameraHost cam;
    int trk_n, trk_B, trk_ready;
    TrackOptions opt;
    // agt_tracker_predict: one allocation made when the option is first switched on: the per-stream pose history (AGT_PRED_* of
    // agt_kernels.h), the frame's flows and the start points of the backward pass of the forward-backward check
    double* pred_hist; float* pred_flow; float* pred_back;
    char* cons_buf; size_t cons_cap;         // scratch of the consensus calls (cons_scratch): hypotheses, and the tracker's inlier bytes / votes
    int* fault_host; int* fault_dev;         // host-mapped word a chained launch sets when a wait gave up (agt_synchronize reports it)
    // agt_track_host_frame: the frame's record and a sequence word in host-mapped memory (same allocation as the fault word: +64 the
    // record, +192 the word); seq(frame t) = hseq_off + t, monotonic across resets and rewinds
    double* hrec_host; double* hrec_dev; unsigned long long* hseq_host; unsigned long long* hseq_dev;
    unsigned long long hseq_off, hseq_last; int host_seq_on;
    // LK parameters of the fused step (COUNT+EPS (30, 0.01), minEig 1e-4, flags 0)
    int lk_max_count; double lk_eps; double lk_min_eig;
    // undistortion maps of the pre-processing stage (built once per camera)
    short2* map1; unsigned short* map2; int map_w, map_h;
    // scratch of the dense refinement: per-block partial sums and the per-stream done words
    double* dense_partials; int* dense_done; size_t dense_cap; int dense_done_B;   // capacities: doubles / streams
    // dense stage of the tracker (agt_tracker_dense): model retained by pointer
    const float* dn_xyz; const float* dn_t; int dn_M, dn_iters, dn_reseed; double dn_weight;
    // optional per-kernel timing (agt_profile_begin/end)
    hipEvent_t* prof_ev;
    int prof_cap, prof_n;
    int* prof_dense;                         // per recorded frame: dense iterations whose launches carry events
};

// bytes between the streams of context-owned level l (>= 1)
inline long level_bstride(const agt_ctx* c, int l) { return (long)c->lh[l] * c->lpitch[l]; }

// agt_api.hip
int hip_fail(agt_ctx* c, hipError_t e);
int fill_camera(const double* K, const double* dist, int ndist, AgtCameraHost* cam, AgtTiltHost* tilt = nullptr);
int camera_on(agt_ctx* c, const double* K, const double* dist, int ndist, AgtCameraHost* cam, bool tracker = false);
int ensure_ring(agt_ctx* c, int want);
int ms_pool_acquire(int device, hipStream_t out[3]);

// agt_tracker_frames.hip
int join_pipeline(agt_ctx* c);            // enqueues the remaining stages of every frame supplied so far
int dense_scratch(agt_ctx* c, size_t need, int B);
int pyramid_build_on(agt_ctx* c, hipStream_t stream, int slot, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B);
void fill_levels(const agt_ctx* c, int slot, AgtLevel* L);          // levels 0 .. eff_max_level of ring entry `slot` (level 0: as registered)
int pyramid_levels_on(agt_ctx* c, hipStream_t stream, int slot, int l0, int B);      // builds levels l0 .. eff_max_level, each from the level below
agt_dense::DenseParams dense_params_on(const agt_ctx* c);           // zeroed, with what every dense call takes from the context: scratch, damping
int lk_track_on(agt_ctx* c, hipStream_t stream, int prev_slot, int next_slot,
                const float* d_prev_pts, const uint8_t* d_prev_status, float* d_next_pts, uint8_t* d_status, float* d_err,
                int n, int B, int crit_type, int crit_max_count, double crit_eps,
                int flags, double min_eig_threshold, int b0 = 0, int waves = 0);
int lk_verdict_on(agt_ctx* c, hipStream_t stream, int prev_slot, int next_slot,
                  const float* d_prev_pts, const float* d_next_pts, uint8_t* d_status, const float* d_err, float* d_fb_dist,
                  int n, int B, int crit_type, int crit_max_count, double crit_eps,
                  int flags, double min_eig_threshold, double fb_max_px, const float* d_back_seed = nullptr);
int lk_lds_min(int per_cu);
// agt_api_calls.hip
// Scratch of one consensus call over B streams of T tags (agt_api_calls.hip): grown when too small, never shrunk
struct ConsScratch { double* hyp_pose; int32_t* hyp_info; double* win; uint8_t* inl; int32_t* votes; };
int cons_scratch(agt_ctx* c, int B, int T, int n, ConsScratch* s);
// hypothesis launch + vote launch on `stream`; fills s.  track != null: the tracker's form (guess per stream from the state; the winner's
// pose stays in scratch).  d_inl / d_votes / d_win null: the scratch arrays.
int consensus_on(agt_ctx* c, hipStream_t stream, const void* d_obj, long obj_bstride, const void* d_img, int dtype, const uint8_t* d_mask,
                 int n, int B, const AgtCameraHost& cam, const double* d_start, int use_guess, const AgtTrackState* track,
                 int cpt, double inlier_px, int min_inliers, uint8_t* d_inl, int32_t* d_votes, double* d_win, ConsScratch* s);
// agt_api_tracker.hip: arguments of the visibility rule (agt_tracker_visibility, agt_tag_visibility): max_view_deg finite in [0, 90], facing +1 / -1, cpt >= 4
bool visibility_args_ok(int corners_per_tag, double max_view_deg, int facing);
double visibility_cos_max(double max_view_deg);                     // cos(max_view_deg), exactly 0 at 90

// Wait for a sequence word in host-mapped memory that a kernel stores behind its results (system scope) to reach `want`; after 2 s
// without it the stream is asked what happened (a launch failed, the device is gone).  Inline: the per-frame caller keeps it in its unit.
inline int poll_seq(agt_ctx* c, const volatile unsigned long long* seq, unsigned long long want)
{
    timespec t0; clock_gettime(CLOCK_MONOTONIC, &t0);
    for (unsigned long spins = 1; *seq < want; spins++) {
#if defined(__x86_64__) || defined(__i386__)
        __builtin_ia32_pause();
#else
        __asm__ __volatile__("" ::: "memory");       // (other hosts: a compiler barrier; the volatile load above is the poll)
#endif
        if ((spins & 0xffff) == 0) {
            timespec t1; clock_gettime(CLOCK_MONOTONIC, &t1);
            if ((t1.tv_sec - t0.tv_sec) + (t1.tv_nsec - t0.tv_nsec) * 1e-9 > 2.0) {
                hipError_t e = hipStreamSynchronize(c->stream);
                if (e != hipSuccess) return hip_fail(c, e);
                if (*seq < want) return AGT_ERR_STATE;
            }
        }
    }
    __atomic_thread_fence(__ATOMIC_ACQUIRE);
    return AGT_OK;
}
