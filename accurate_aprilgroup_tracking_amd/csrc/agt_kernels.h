// agt_kernels.h -- host-visible launch interface of the gfx950 kernels (internal to the library).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <cstddef>
#include <type_traits>
#include "../../include/agt_hip.h"

struct AgtLevel {
    const uint8_t* ptr;   // level base for stream 0
    long pitch;           // bytes per row (multiple of 4)
    long bstride;         // bytes between streams
    int w, h;
};

// ---- the chip a context runs on (round 5: no literal 8 XCDs / 256 CUs in kernels or launch rules).
// Workgroups of a launch are dealt round-robin to the XCDs, each with its own L2; the kernels that re-use lines between
// neighbouring work items (pyramid tiles / strips, LK corners of a stream, undistortion bands) re-order their block index so
// that every XCD walks a CONTIGUOUS run of items:  item = (b mod X) * (n / X) + b / X  for a grid of n blocks, n a multiple of
// X = 2^xshift.  A pure index map (a permutation of 0 .. n - 1 for every X): correct on any device, tuned when X is the device's
// XCD count.  gfx950: one XCD = 32 CUs (MI355X: 256 CUs = 8 XCDs; its CPX / QPX / DPX partitions: 32 / 64 / 128 CUs = 1 / 2 / 4).
struct AgtChip {
    int cus;                  // hipDeviceProp_t::multiProcessorCount
    int xcds;                 // 1, 2, 4 or 8 (cus / 32 when that is a power of two, else 1: plain order)
    int xshift;               // log2(xcds)
    char arch[32];            // gcnArchName up to the first ':'
};
// gfx950: 160 KB of LDS per CU (MI355X_MICROARCH.md; hipDeviceProp_t reports the 64 KB a workgroup may ask for, not this)
constexpr long AGT_LDS_PER_CU = 160L * 1024;
__host__ __device__ inline int agt_xcd_order(int b, int nblk, int xshift)
{
    return (b & ((1 << xshift) - 1)) * (nblk >> xshift) + (b >> xshift);
}
inline unsigned agt_xcd_grid(long items, int xshift) { const long x = 1L << xshift; return (unsigned)((items + x - 1) / x * x); }
const AgtChip* agt_chip_of(int device);        // cached device query (agt_api.hip); null when the query fails
const AgtChip& agt_chip_current(void);         // of the calling thread's current device; MI355X's figures if the query fails

struct AgtPyrArgs {
    const uint8_t* src; uint8_t* dst;
    long spitch, sbatch, dpitch, dbatch;
    int sw, sh, dw, dh;
    int gx, gy, B;            // tiled form: tile grid (x, y); register-rolling form: gx = workgroups per image, gy = 1.  B: images
    int strip_rows;           // output rows per strip of the register-rolling form (two-level pass: level-2 rows); 0 = tiled form
    int xshift;               // log2 of the XCD count the block order is laid out for (agt_xcd_order); set by the launchers
    int topdown;              // two-level rolling pass: 1 = every strip top-down (diagnostic A/B; 0 = alternating directions)
};
__host__ __device__ inline bool agt_pyr_rolling(const AgtPyrArgs& A) { return A.strip_rows != 0; }
__host__ __device__ inline int agt_pyr_blocks(const AgtPyrArgs& A) { return A.gx * A.gy; }        // workgroups per image, either form
// (the device reads these members from the kernel-argument segment by offset: agt_step.hip pyr_role)
#define AGT_PYR_AT(m, o) static_assert(offsetof(AgtPyrArgs, m) == o, "AgtPyrArgs layout: " #m)
AGT_PYR_AT(src, 0); AGT_PYR_AT(dst, 8); AGT_PYR_AT(spitch, 16); AGT_PYR_AT(sbatch, 24); AGT_PYR_AT(dpitch, 32); AGT_PYR_AT(dbatch, 40);
AGT_PYR_AT(sw, 48); AGT_PYR_AT(sh, 52); AGT_PYR_AT(dw, 56); AGT_PYR_AT(dh, 60); AGT_PYR_AT(gx, 64); AGT_PYR_AT(gy, 68); AGT_PYR_AT(B, 72);
AGT_PYR_AT(strip_rows, 76); AGT_PYR_AT(xshift, 80); AGT_PYR_AT(topdown, 84);
#undef AGT_PYR_AT
static_assert(sizeof(AgtPyrArgs) == 88, "AgtPyrArgs layout");

#define AGT_MAX_GROUP 32         // frames one fused launch may advance each pipeline stage by (the per-frame tables are kernel arguments: 7.4 KB with the parameters)

// Forward-backward check (agt_lk_track_fb, agt_tracker_fb_check): the BACKWARD launch of the stand-alone LK kernels -- slots swapped,
// prev_pts = the forward result q, prev_status = status = the forward status -- runs in verdict mode: it publishes no point and no err;
// a corner whose round trip does not come home within max_px of orig has its status byte cleared (agt_lk_body.h lk_publish).
struct AgtLkVerdict {
    const float* orig;        // [B][n][2] the points the forward pass started from; null = an ordinary launch
    float* dist;              // [B][n] round-trip distance (-1 where either pass lost the corner), or null
    float max_px;             // a corner is kept while max(|dx|, |dy|) < max_px
    int pad_;
};

#define AGT_LK_FLAG_GENERAL  0x10000    // internal launch flags: the general body for every corner (diagnostic: AGT_LK_RS=0) ...
#define AGT_LK_FLAG_COTENANT 0x20000    // ... the context declared co-tenancy (agt_lk_occupancy_cu): tracker waves at issue priority 1
struct AgtLkParams {
    AgtLevel prev[AGT_MAX_LEVELS];
    AgtLevel next[AGT_MAX_LEVELS];
    int max_level;            // effective (after OpenCV's early stop)
    int n;                    // points per stream
    int max_count;            // criteria, already clamped
    double eps2;              // epsilon^2
    int flags;                // AGT_LK_* of the ABI in the low bits; internal: AGT_LK_FLAG_GENERAL, AGT_LK_FLAG_COTENANT
    double min_eig_threshold;
    const float* prev_pts;    // [B][n][2]
    const uint8_t* prev_status;   // [B][n] or null: tracker mode, a corner lost in an earlier frame stays lost (position carried)
    float* next_pts;          // [B][n][2]
    uint8_t* status;          // [B][n]
    float* err;               // [B][n] or null
    int xshift;               // XCD-aware corner order (agt_xcd_order); set by the launchers
    int lds_min;              // host side only: least dynamic LDS a one-wave workgroup asks for = a residency cap (agt_lk_occupancy_cu); 0 = none
    AgtLkVerdict fb;          // forward-backward verdict launch (fb.orig != null); all zero otherwise.  Three words, as ever: the size
                              // keeps the kernel-argument offsets of the structures that embed this one
};
static_assert(sizeof(AgtLkVerdict) == 24, "AgtLkVerdict fills the three reserved words of AgtLkParams");

struct AgtCameraHost {
    double fx, fy, cx, cy;
    double k[12];
    // tilted sensor (coefficients 13, 14 = tau_x, tau_y; round 5): DEVICE pointer to matTilt | invMatTilt (2 x 9 doubles, row-major, as
    // detail::computeTiltProjectionMatrix builds them), null without tilt.  In global memory, not in this by-value struct: loads from the
    // kernel-argument segment are speculated in front of the `if (tilt)` branches and the 36 scalar registers they fill cost the fused
    // step kernel 86 more spilled SGPRs (measured); a load through a pointer that may be null stays inside its branch.
    const double* tilt;
};
// the same matrices on the host (agt_api.hip fill_camera): m = matTilt | invMatTilt, on = 0: identities
struct AgtTiltHost { double m[18]; int on; };

struct AgtPnpParams {
    const void* obj;          // n x 3, f32 or f64
    long obj_bstride;         // elements between streams (0 = shared)
    const void* img;          // [B][n][2]
    const uint8_t* mask;      // [B][n] or null
    int dtype;                // AGT_F32 / AGT_F64 (img and obj)
    int img_f32_obj_f32;      // unused, keeps layout explicit
    int n;
    int use_guess;
    AgtCameraHost cam;
    double* pose;             // [B][6] in/out
    int32_t* info;            // [B][4] or null
    double* err;              // [B] or null
    // tracker mode (null = plain solvePnP): PoseDetector._estimate_pose on device state
    struct AgtTrackState* track;   // [B]
    double* state_out;             // [B][AGT_STATE_STRIDE] or null
    float* corners_rw;             // [B][n][2] corner set to refresh by reprojection, or null
    uint8_t* status_rw;            // [B][n] LK status revived together with corners_rw, or null
    // dense stage hand-over (agt_track_frame_dense): start pose, done word (1 = pose not accepted: skip) and the frame's record
    double* dense_pose;            // [B][6] or null
    int* dense_done;               // [B]
    double* dense_rec;             // [B][AGT_DENSE_STRIDE]
    int enhance_ape;
    int reproject;
    int min_points;                // corners needed to attempt a pose (8 = two tags)
    double gate_px;                // reprojection gate (2.0, detect_pose.py:539)
    int tag_gate;                  // 4: a corner counts only while all four corners of its tag are usable (the reference solves on
                                   // whole tags, detect_pose.py:400-437, :494-496); 0: every usable corner counts
    int pad_;
    int* fault;                    // chained launch: host-mapped word set to 1 when a wait gave up (agt_synchronize reports it), or null
    float* seed_pts;               // agt_track_frame_detected: the detector's corner table (img, mask) becomes the frame's corner set
    uint8_t* seed_status;          // / LK status ([B][n][2], [B][n]: the tracker's ring entry of the frame), or null
    // agt_track_host_frame: host-mapped sequence word the solver of stream 0 stores (system scope) behind the frame's record -- whose
    // destination is host-mapped too -- so that the calling thread can poll for the record instead of waiting for the stream;
    // frame k of a launch stores host_seq_base + k.  null: off.
    unsigned long long* host_seq;
    unsigned long long host_seq_base;
    // agt_tracker_visibility (vis_cpt != 0: on): the reproject refresh revives the corners of visible tags only (agt_device.h agt_tag_visible;
    // tag t = corners vis_cpt * t ..) and clears the status of the others; read by the tracker-mode launches of agt_pnp.hip alone
    double vis_cos_max;            // cos(max_view_deg); exactly 0 at 90 degrees
    int vis_cpt;                   // corners per tag (>= 4; n / vis_cpt <= 64: one ballot holds the verdicts), 0 = rule off
    int vis_facing;                // +1 / -1: the tag normal is facing * (p3 - p0) x (p1 - p0)
    // Tag consensus (agt_solve_pnp_consensus, agt_tracker_consensus); read by the launches of agt_pnp.hip alone (template flag CONS).
    // Hypothesis launch (hyp_T != 0): problem g of the grid is tag g % hyp_T of stream s = g / hyp_T -- n is the corner count of ONE tag,
    // img / mask / pose / info / err are indexed by g ([B * hyp_T][n] views of the caller's [B][n * hyp_T] arrays), the object points are
    // obj + s * obj_bstride + (g % hyp_T) * n * 3, and the solve starts from hyp_pose[s] (use_guess) or, in the tracker, from
    // hyp_track[s].guess when that stream has a guess and enhance_ape is set (which then decides use_guess per stream).
    int hyp_T;
    int pad2_;
    const double* hyp_pose;                  // [B][6] or null: start from pose[g]
    const struct AgtTrackState* hyp_track;   // [B] or null
    // Pose step of the tracker under the option: a corner is used while mask AND cons_inl say so; the record's AGT_ST_NINLIER slot
    // carries cons_votes[b][1].  Both null: off.
    const uint8_t* cons_inl;                 // [B][n]
    const int32_t* cons_votes;               // [B][4]
    // agt_tracker_predict (null: off): the stream's block of the pose history, AGT_PRED_STRIDE doubles (layout below).  The pose step files
    // the pose and the verdict of EVERY record it writes in the block's `last` entry and copies the flow word into the record's AGT_ST_FLOW
    // slot; read by the launches of agt_pnp.hip alone (template flag CONS)
    double* pred_hist;                       // [B][AGT_PRED_STRIDE]
};
// Pose history of agt_tracker_predict, per stream: the record the pose step wrote last (pose, accepted), the flow word of the frame (the seed
// launch's flow_max, handed to the pose launch), and the record before that one.  The seed launch (flow_kernel, agt_project.hip) predicts
// from the two entries while both are accepted, then moves `last` to `before` and clears `last`.
#define AGT_PRED_STRIDE 16
#define AGT_PRED_LAST   0     // 0..5 pose, 6 accepted (1.0 / 0.0)
#define AGT_PRED_FLOW   7
#define AGT_PRED_BEFORE 8     // 8..13 pose, 14 accepted

// device-resident per-stream tracker state: the attributes of PoseDetector
// (detect_pose.py:74-83) that _estimate_pose mutates
struct AgtTrackState {
    double guess[6];        // extrinsic_guess (rvec, tvec)
    double prev[6];         // prev_transform
    double rot_vel[2][9];   // rot_velocities (oldest first)
    double tran_vel[2][3];  // tran_velocities
    double prev_R[9];       // Rodrigues(prev rvec), kept from the solve that produced prev (device cache, not reference state)
    int has_guess;          // extrinsic_guess[0] is not None
    int has_prev;           // prev_transform[0] is not None
    int n_vel;              // len(rot_velocities)
    int frame;
    int guess_t_f32;        // dtype of extrinsic_guess[1] is float32 (from get_rmat_tvec, transform_helper.py:158-159)
    int prev_t_f32;         // dtype of prev_transform[1] is float32
    int chain_fault;        // sticky: a chained launch gave up waiting for this stream's corners (AGT_TRK_CHAIN_TIMEOUT); the stream's
                            // state is frozen and every later record is flagged invalid until agt_tracker_reset
    int pad;
};

// one fused launch (agt_step.hip): block ranges [LK | PnP | pyr stage 0 | stage 1 | ..]; every role advances
// by up to AGT_MAX_GROUP consecutive frames (the LK and PnP roles loop over them inside the launch: their
// chains are serial across frames; the pyramid stages treat the frames as a batch)
struct AgtStepParams {
    AgtPyrArgs pyr[AGT_MAX_LEVELS - 1];                        // geometry; src / dst per frame in AgtStepTables
    int pyr_fused;                    // != 0: stage 0 builds levels 1 AND 2 in one pass (agt_step_set_two_level); stage 1 then has no blocks
    int pyr_pad;
    int pyr_nf[AGT_MAX_LEVELS - 1];
    int n_pyr[AGT_MAX_LEVELS - 1];    // blocks of each pyramid stage = tiles x streams x frames (0 = stage idle)
    AgtLkParams lk;                   // geometry of prev[] / next[], criteria; images per frame in AgtStepTables
    int lk_nf;
    int n_lk;                         // != 0: LK role active (block count is derived at launch)
    int lk_B;                         // streams of the LK role
    AgtPnpParams pnp;
    int pnp_nf;
    int n_pnp;                        // blocks of the PnP role (= streams) or 0
    int xshift;                       // XCD-aware block orders of the LK and pyramid roles (agt_xcd_order); set by the launchers
    int rsv_;
};
// Stage 0 as the two-level pass: A[0] = the level 0 -> 1 half, which also carries the pass's grid (agt_pyr2_plan), A[1] = the level 1 -> 2
// half, which rides in stage 1's slots (pyr[1]; its level-2 buffers per frame in AgtStepTables::pyr_dst[1])
inline void agt_step_set_two_level(AgtStepParams& S, const AgtPyrArgs* A) { S.pyr[0] = A[0]; S.pyr[1] = A[1]; S.pyr_fused = 1; }

// per-frame pointer tables of the fused launch: its SECOND kernel argument.  They are indexed with run-time
// frame numbers and therefore read from the kernel-argument segment directly (never through a by-value copy).
struct AgtLkTables {
    const uint8_t* img[AGT_MAX_GROUP + 1][AGT_MAX_LEVELS];     // image k of the group per level (k = 0: the frame before it)
    float* next[AGT_MAX_GROUP];                                // frame k+1's corners / status
    uint8_t* status[AGT_MAX_GROUP];
    unsigned* done[AGT_MAX_GROUP];                             // chained launch: arrival counters of frame k+1 ([B], one count per corner) or null
};
struct AgtPnpTables {
    const float* img[AGT_MAX_GROUP];                           // per frame: corners, LK status, caller's state record
    const uint8_t* mask[AGT_MAX_GROUP];
    double* so[AGT_MAX_GROUP];
    const unsigned* wait[AGT_MAX_GROUP];                       // chained launch: the frame's LK arrival counters ([B]) or null = complete before the launch
    unsigned long long target[AGT_MAX_GROUP];                  // counter value that means "all corners of the frame are written"
};
struct AgtStepTables {
    const uint8_t* pyr_src[AGT_MAX_LEVELS - 1][AGT_MAX_GROUP];
    uint8_t* pyr_dst[AGT_MAX_LEVELS - 1][AGT_MAX_GROUP];
    AgtLkTables lk;
    AgtPnpTables pnp;
};

// ---- the projection family (agt_project.hip): one argument block and one launcher per job.  obj / obj_bstride / dtype / n are the object
// points as in AgtPnpParams (n per stream, obj_bstride elements between streams, 0 = shared).
// cv::projectPoints: thread i of stream b's blocks projects point i under pose[b]
struct AgtPointsParams {
    const void* obj; long obj_bstride; int dtype; int n;
    const double* pose;       // [B][6]
    AgtCameraHost cam;
    void* img_out;            // [B][n][2]
    double* jac;              // [B][2n][6] or null
    // agt_project_points_host (one block, B = 1): host-mapped sequence word stored behind the outputs (see AgtPnpParams::host_seq); null: off
    unsigned long long* host_seq;
    unsigned long long host_seq_base;
};
// agt_tag_visibility: thread i of stream b's blocks judges tag i (object points vis_cpt * i ..) under pose[b] with agt_tag_visible
struct AgtVisibleParams {
    const void* obj; long obj_bstride; int dtype; int n;
    const double* pose;       // [B][6]
    uint8_t* vis_out;         // [B][n / vis_cpt]
    double* vis_cos;          // [B][n / vis_cpt] or null
    double vis_cos_max;
    int vis_cpt, vis_facing;
};
// agt_solve_pnp_consensus: ONE workgroup per stream, thread i owns corner i (n <= 256, n / vote_cpt <= 64).  Every usable corner is
// projected under every accepted hypothesis (vote_pose / vote_info: the hypothesis launch's results, [B][T][6] / [B][T][4],
// T = n / vote_cpt); the workgroup elects the hypothesis with the most inliers and writes the stream's inlier bytes, its votes row and,
// when there is a consensus, the winner's pose to vote_win[b].
struct AgtVoteParams {
    const void* obj; long obj_bstride; int dtype; int n;
    AgtCameraHost cam;
    const void* vote_img;     // [B][n][2], dtype as obj
    const uint8_t* vote_mask; // [B][n] or null
    const double* vote_pose;
    const int32_t* vote_info;
    uint8_t* vote_inl;        // [B][n]
    int32_t* vote_votes;      // [B][4] or null: winning tag (-1: none), its inlier count (0: none), candidate tags, accepted hypotheses
    double* vote_win;         // [B][6]
    double vote_tau2;         // inlier_px^2
    int vote_cpt, vote_min;
};
// agt_predict_flow, agt_tracker_predict: ONE workgroup per stream, thread i owns corner i (n <= 256).  The constant-velocity
// extrapolation of the poses flow_older[b] -> flow_newer[b] (stride flow_pstride doubles) is computed once per workgroup, every usable
// corner is projected under the newer and the predicted pose, the workgroup decides whether the prediction is trusted and writes seeds,
// flows, flow_max and the predicted pose (the rule: include/agt_hip.h).  flow_hist != null: the tracker's form -- the poses are the two
// entries of the stream's history block (AGT_PRED_*; flow_older / flow_newer are not read), a stream whose entries are not both accepted
// has no prediction (seeds = flow_prev, flow_max 0), and the block is advanced for the frame's pose step.  n = 0 with flow_hist: only that.
struct AgtFlowParams {
    const void* obj; long obj_bstride; int dtype; int n;
    AgtCameraHost cam;
    const double* flow_older; // [B][6]
    const double* flow_newer;
    long flow_pstride;
    const float* flow_prev;   // [B][n][2]
    const uint8_t* flow_mask; // [B][n] or null
    float* flow_seed;         // [B][n][2]
    float* flow_out;          // [B][n][2] or null
    float* flow_max;          // [B] or null
    double* flow_pred;        // [B][6] or null
    double* flow_hist;        // [B][AGT_PRED_STRIDE] or null
    float flow_cap;           // (float)max_flow_px
};
// the tracker's forward-backward check under agt_tracker_predict: thread i of stream b's blocks writes
// flow_back[b][i] = flow_prev[b][i] - flow_out[b][i] (float32), where the backward LK pass starts
struct AgtFlowBackParams {
    int n;
    const float* flow_prev;   // [B][n][2]
    const float* flow_out;    // [B][n][2]
    float* flow_back;         // [B][n][2]
};

// The dense stage's parameter block (agt_dense.hip: specification, mapping; agt_dense_body.h: the update).  The caller fills frame, model,
// corner set, camera, pose, scratch (partials, done) and weights; agt_launch_dense derives the rest.
namespace agt_dense {
struct DenseParams {
    const uint8_t* img; long pitch, ibatch; int w, h;
    const float* mxyz; const float* mt; int M;
    const float* obj; const float* ipts; const uint8_t* mask; int N;
    AgtCameraHost cam;
    double* pose;                      // [B][6]
    double* partials;                  // [2][B][nblk + 1][DROW]: block rows, double-buffered by iteration parity
    double* ppose;                     // [2][B][8]: linearisation point of iteration k + 1 (published by block 0 of launch k + 1)
    long pstride;                      // doubles between the two row buffers
    int nblk;
    double* stats;                     // [B][stats_stride]: 5 values written per iteration
    int stats_stride;
    double* rec;                       // tracker stage: per-frame record [B][AGT_DENSE_STRIDE] (pose, refined flag, stats) or null
    int* done;                         // [B]
    double photo_weight, mu;
    int iter;
    float* seed_pts; uint8_t* seed_status;     // tracker stage with re-seed: the frame's corner set / LK status ([B][N][2], [B][N]) or null
    // clip submission (agt_track_frames_dense): the two-level pyramid pass of the NEXT frame rides in the first accumulate launch
    // as extra workgroups (blockIdx.x > nblk) -- it depends on nothing this frame computes, and alone it was a 6.5 us launch
    // in the frame's serial chain
    AgtPyrArgs py0, py1;
    int n_pyr;                                 // tiles per stream (0 = none)
};
}  // namespace agt_dense

// The source-side view of agt_preproc.hip's RemapParams (the kernel's argument): what agt_launch_preprocess is given
struct AgtRemapArgs {
    const uint8_t* src; long spitch, sbatch; int sw, sh;
    const short2* map1; const unsigned short* map2; int mw;      // maps cover mw x (any) pixels
    int rx, ry, rw, rh;                                          // output window in map coordinates
    uint8_t* dst; long dpitch, dbatch;
    int undistort;                                               // 0: taps come straight from (x, y)
    int B;                                                       // images (gray path: flattened work order)
    int xshift;                                                  // log2 of the XCD count the gray path's band order is laid out for; set by the launcher
};

// The two compiled pyramid depths of the LK kernels: NLEV = 3 for max_level < 3, AGT_MAX_LEVELS beyond.  f(std::integral_constant<int, NLEV>)
template <class F> inline auto agt_with_nlev(int max_level, F&& f)
{
    return max_level < 3 ? f(std::integral_constant<int, 3>()) : f(std::integral_constant<int, AGT_MAX_LEVELS>());
}

void agt_pyr_grid(int dw, int dh, int* gx, int* gy);
void agt_pyr_plan(AgtPyrArgs* A, uintptr_t src_align, uintptr_t dst_align, int frames);     // tiled or register-rolling form of one pyrDown pass (agt_pyramid.hip)
hipError_t agt_launch_pyr_upload2(hipStream_t stream, const uint8_t* src, int sw, int sh, long spitch, uint8_t* copy, long cpitch,
                                  uint8_t* dst1, long dpitch1, uint8_t* dst2, long dpitch2);     // fused upload + two-level pyramid of one frame (agt_pyramid.hip)
// The two-level pass lv[0] -> lv[1] -> lv[2] as the pair of argument blocks A[0], A[1] its body takes: the geometry (tiled form) ...
void agt_pyr2_args(const AgtLevel* lv, int B, AgtPyrArgs* A);
void agt_pyr2_plan(AgtPyrArgs* A, uintptr_t src_align, uintptr_t dst_align, int frames, int oh_cap = 16);     // ... its form (tiled or register-rolling) ...
hipError_t agt_launch_pyr_down2(hipStream_t stream, const AgtPyrArgs* A);                                     // ... and the launch of what was planned
void agt_pyr2_grid(int w2, int h2, int* gx, int* gy);           // tile grid of the two-level pass (64 x 16 tiles of L2)
hipError_t agt_launch_pyr_down(hipStream_t stream, const AgtLevel& src, const AgtLevel& dst, int B);          // dst.w, dst.h are implied: (w + 1) / 2
// waves: 0 = by batch size (agt_lk_wide), 1 / 4 = that many waves per corner (win 21 only)
hipError_t agt_launch_lk(hipStream_t stream, const AgtLkParams& p, int win, int B, int waves = 0);
// ride != null (two argument blocks of agt_pyr2_args): the two-level pyramid pass of another frame as extra workgroups of the
// launch; only where agt_pnp_can_ride(n) (the four-wave kernel of n > 64)
hipError_t agt_launch_pnp(hipStream_t stream, const AgtPnpParams& p, int B, const AgtPyrArgs* ride = nullptr);
bool agt_pnp_can_ride(int n);
// each refuses what its kernel cannot do (vote: n > 256, vote_cpt <= 0, more than 64 tags; flow: n > 256, n > 0 without seeds)
hipError_t agt_launch_points(hipStream_t stream, const AgtPointsParams& p, int B);
hipError_t agt_launch_visible(hipStream_t stream, const AgtVisibleParams& p, int B);
hipError_t agt_launch_vote(hipStream_t stream, const AgtVoteParams& p, int B);
hipError_t agt_launch_flow(hipStream_t stream, const AgtFlowParams& p, int B);
hipError_t agt_launch_flow_back(hipStream_t stream, const AgtFlowBackParams& p, int B);
hipError_t agt_launch_undistort_map(hipStream_t stream, const double* K, const AgtCameraHost& cam, const AgtTiltHost& tilt, const double* ir,
                                    int w, int h, short2* map1, unsigned short* map2);
hipError_t agt_launch_preprocess(hipStream_t stream, const AgtRemapArgs& A, int gray);
// The dense stage's last step (final Gauss-Newton update + corner re-seed) handed on to the LK launch of the NEXT frame instead of
// being launched: the stage's parameter block as agt_launch_dense left it (agt_step_dense.hip agt_launch_lk_reseed reads it)
struct AgtDenseFinal { agt_dense::DenseParams P; };
hipError_t agt_launch_lk_reseed(hipStream_t stream, const struct AgtStepParams& S, const struct AgtStepTables& T, int win, const AgtDenseFinal* F, const struct AgtPyrArgs* ride = nullptr);
hipError_t agt_launch_dense_final(hipStream_t stream, const AgtDenseFinal& F, int B);      // the deferred step as its own launch after all
// P.rec == null: plain agt_dense_refine (done words cleared here, P.stats [B][8]).  P.rec != null: stage of the tracker -- the done words
// and the start poses were written by the PnP epilogue of the same frame (done = pose not accepted), the statistics go into the record;
// P.seed_pts / seed_status != null: the corner re-seed rides in the final launch.  P.partials: agt_dense_doubles(M, B) doubles.
// ev: profiling events; next_pyr: the riding two-level pass (agt_pyr2_args); defer_final: the last step is left there, not launched
hipError_t agt_launch_dense(hipStream_t stream, agt_dense::DenseParams P, int B, int iters,
                            hipEvent_t* ev = nullptr, int n_ev = 0, const AgtPyrArgs* next_pyr = nullptr, AgtDenseFinal* defer_final = nullptr);
int agt_dense_blocks(int M);
size_t agt_dense_doubles(int M, int B);
bool agt_lk_window_supported(int win);
void agt_lk_window_size(int win, int* ww, int* wh);       // AgtConfig::win -> (width, height): a side, or AGT_WIN_RECT(w, h)
bool agt_lk_wide(int n, int B);
bool agt_step_supported(int win);
bool agt_step_fits(int n, int B);   // the fused launch (all roles in one kernel) is used while its LK workgroups fit one per CU (256 corners on a whole MI355X)
// role subsets of one pipeline group (split mode launches them separately, each with its own LDS size and register budget)
#define AGT_STEP_PYR 1
#define AGT_STEP_LK  2
#define AGT_STEP_PNP 4
#define AGT_STEP_ALL 7
hipError_t agt_launch_step(hipStream_t stream, const AgtStepParams& S, const AgtStepTables& T, int win, int roles);
