// agt_tracker.h -- what the tracker's host units share (agt_api_tracker.hip: the entry points; agt_api_live.hip: the live camera loop;
// agt_tracker_frames.hip: what a tracked frame is issued with -- the stages, the pipelined launch form, fused or split, and the serial
// step).  What the stateless calls use as well is declared in agt_ctx.h.  Nothing here leaves the library.
#pragma once
#include "agt_ctx.h"
#include <string.h>

// ---- the idioms of the units, inline on the per-frame path: ring entry of tracker frame `frame`; level l of the pyramid in ring entry
// `slot` (level 0 is the caller's frame)
static inline int ring_slot(const agt_ctx* c, long frame) { return (int)(frame % c->live_ring); }
static inline const uint8_t* level_ptr(const agt_ctx* c, int slot, int l) { return l == 0 ? c->frame[slot].ptr : c->lmem[slot][l]; }
static inline bool frame_args_ok(const agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride)
{
    return !((pitch & 3) || ((uintptr_t)d_frames & 3) || (batch_stride & 3) || pitch < (size_t)c->cfg.width);
}
// A frame takes ring entry `slot`: level 0 is the caller's buffer, B streams of it; state_out: where its record goes (fused pipeline).
// (pyramid_build_on registers the same, but B only once its launches are out.)
static inline void register_frame(agt_ctx* c, int slot, const uint8_t* ptr, size_t pitch, size_t batch_stride, int B, double* state_out)
{
    c->frame[slot] = RingFrame{ ptr, (long)pitch, (long)batch_stride, B, state_out };
}
// frame t is the newest frame and complete in every stage
static inline void frame_complete(agt_ctx* c, long t)
{
    c->trk_frame = c->n_lk = c->n_pnp = t;
    for (int s = 0; s < AGT_MAX_LEVELS; s++) c->n_stage[s] = t;
}
// stage spans are being recorded (agt_profile_begin) and there is room for another frame's; that frame's events (null: none)
static inline bool profiling_armed(const agt_ctx* c) { return c->prof_ev && c->prof_n < c->prof_cap; }
static inline hipEvent_t* profile_events(const agt_ctx* c) { return profiling_armed(c) ? c->prof_ev + (size_t)c->prof_n * AGT_PROF_EVENTS : nullptr; }

// ---- agt_tracker_frames.hip (join_pipeline and what the stateless calls use as well: agt_ctx.h): the pose step, the two launch forms
void fill_estimate(const agt_ctx* c, AgtPnpParams* p, const float* d_img, const uint8_t* d_mask,
                   double* d_state_out, float* corners_rw, uint8_t* status_rw = nullptr);
int pose_step_on(agt_ctx* c, hipStream_t stream, AgtPnpParams* p, int B, int prev_slot, const AgtPyrArgs* ride = nullptr);
int step_pipelined(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B, double* d_state_out);
int step_pipelined_uploaded(agt_ctx* c, const uint8_t* h_dev, uint8_t* d_gray, size_t gpitch, double* d_state_out);
void ring_move(agt_ctx* c, long f, int old_ring, int new_ring);
int step_serial(agt_ctx* c, const uint8_t* d_frames, size_t pitch, size_t batch_stride, int B,
                double* d_state_out, double* d_dense_out, hipEvent_t* pev, const uint8_t* next_frame = nullptr);
