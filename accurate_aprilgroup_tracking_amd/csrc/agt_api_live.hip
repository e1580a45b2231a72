// agt_api_live.hip -- the live camera loop of the C ABI: the per-frame pre-processing call and agt_track_host_frame, one call from a
// host frame to its record on the host (with the timing knob of the diagnostic libraries).
#include "agt_tracker.h"
#include <stdio.h>

// undistort (optional) + BGR2GRAY + ROI crop in one pass: BGR (src_w x src_h) -> gray (roi_w x roi_h)
int agt_preprocess_bgr(agt_ctx* c, const uint8_t* d_bgr, size_t spitch, size_t sbatch, int src_w, int src_h, int B,
                       int undistort, int roi_x, int roi_y, int roi_w, int roi_h,
                       uint8_t* d_gray, size_t gpitch, size_t gbatch)
{
    if (!c || !d_bgr || !d_gray || B <= 0 || src_w <= 0 || src_h <= 0) return AGT_ERR_ARG;
    if (roi_x < 0 || roi_y < 0 || roi_w <= 0 || roi_h <= 0 || roi_x + roi_w > src_w || roi_y + roi_h > src_h) return AGT_ERR_ARG;
    if (spitch < (size_t)src_w * 3 || gpitch < (size_t)roi_w) return AGT_ERR_ARG;
    if (undistort && (!c->map1 || c->map_w != src_w || c->map_h != src_h)) return AGT_ERR_STATE;
    AgtRemapArgs A = AgtRemapArgs();
    A.src = d_bgr; A.spitch = (long)spitch; A.sbatch = (long)sbatch; A.sw = src_w; A.sh = src_h; A.map1 = c->map1; A.map2 = c->map2; A.mw = src_w;
    A.rx = roi_x; A.ry = roi_y; A.rw = roi_w; A.rh = roi_h; A.dst = d_gray; A.dpitch = (long)gpitch; A.dbatch = (long)gbatch;
    A.undistort = undistort ? 1 : 0; A.B = B;
    hipError_t e = agt_launch_preprocess(c->stream, A, 1);
    return e == hipSuccess ? AGT_OK : hip_fail(c, e);
}

// The live camera loop in ONE call (detect_pose.py:669-681, LK path): host frame -> HBM -> [undistort / gray / crop] -> agt_track_frame
// -> join -> record back -> wait.  Everything a Python caller would otherwise issue as five separate foreign calls.
int agt_track_host_frame(agt_ctx* c, const uint8_t* h_frame, int channels, int src_w, int src_h, uint8_t* d_staging,
                         int undistort, int roi_x, int roi_y, uint8_t* d_gray, size_t gpitch, double* d_state, double* h_state)
{
    if (!c || !h_frame || !d_gray || !h_state || (channels != 1 && channels != 3)) return AGT_ERR_ARG;
    if (c->trk_ready != 2 || c->trk_B != 1) return AGT_ERR_STATE;
    const int W = c->cfg.width, H = c->cfg.height;
    hipError_t e;
#ifdef AGT_DEBUG_KNOBS      // diagnostic library only: AGT_HOST_FRAME_TIMES=1 prints where the host time of this call goes (us, mean) at exit
    struct Acc { double t[6]; long n; ~Acc() { if (n) fprintf(stderr, "agt_track_host_frame host us: upload-call %.2f track-call %.2f join %.2f d2h-call %.2f sync %.2f total %.2f (n=%ld)\n",
                                                              t[0] / n, t[1] / n, t[2] / n, t[3] / n, t[4] / n, t[5] / n, n); } };
    static Acc acc = {};
    const long timing = AGT_KNOB("AGT_HOST_FRAME_TIMES", 0);
    auto now = [] { timespec ts; clock_gettime(CLOCK_MONOTONIC, &ts); return ts.tv_sec * 1e6 + ts.tv_nsec * 1e-3; };
    double tq[6] = { 0, 0, 0, 0, 0, 0 };
    if (timing) tq[0] = now();
#define AGT_TQ(i) do { if (timing) tq[i] = now(); } while (0)
#else
#define AGT_TQ(i)
#endif
    // Polled record: the frame's record goes straight to host-mapped memory of the context and the solver stores a sequence word behind
    // it (system scope); this thread polls the word -- no 128-byte copy (a blit KERNEL of ~4.5 us behind the step's launch,
    // rocprofv3), no completion signal, no stream wait.  (With profiling spans armed the call waits for the stream as before.)
    const bool polled = !profiling_armed(c);
    double* const d_rec = (polled || !d_state) ? c->hrec_dev : d_state;       // where the pose solver writes the frame's record
    bool registered = false;
    // (the device address of the caller's buffer when it is pinned host memory, asked for on EVERY call: a cached answer would outlive the buffer)
    const uint8_t* h_dev = nullptr;
    {
        hipPointerAttribute_t at;
        if (hipPointerGetAttributes(&at, h_frame) == hipSuccess && at.type == hipMemoryTypeHost) h_dev = (const uint8_t*)at.devicePointer;
        else (void)hipGetLastError();
    }
    if (channels == 1) {
        if (src_w != W || src_h != H || roi_x || roi_y || undistort) return AGT_ERR_ARG;
        // Round 4: a gray frame in PINNED host memory is not copied first: the two-level pyramid pass reads it over PCIe and writes its
        // level 0 to d_gray on the way (step_pipelined_uploaded) -- one launch instead of a copy-engine transfer (19 us + ~8 us of
        // submission and hand-over) and a pyramid launch (6 us).  Pageable memory, frame sizes the rolling pass does not take, the
        // stage-by-stage mode and pending pyramid work of earlier frames keep the copy.
        if (h_dev && polled && c->pipeline && !c->opt.stage_by_stage() && agt_step_fits(c->trk_n, 1)) {
            int rcu = step_pipelined_uploaded(c, h_dev, d_gray, gpitch, d_rec);
            if (rcu < 0) return rcu;
            registered = rcu == AGT_OK;
        }
        if (!registered) {
            if (gpitch == (size_t)W) e = hipMemcpyAsync(d_gray, h_frame, (size_t)W * H, hipMemcpyHostToDevice, c->stream);
            else e = hipMemcpy2DAsync(d_gray, gpitch, h_frame, (size_t)W, (size_t)W, (size_t)H, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) return hip_fail(c, e);
        }
    } else {
        // BGR: without undistortion the gray conversion streams through the frame once -- from pinned host memory it reads the frame
        // over PCIe itself (no 2.8 MB copy first); the undistortion's gather keeps the frame in HBM (d_staging)
        const uint8_t* src = d_staging;
        if (h_dev && !undistort) src = h_dev;
        else {
            if (!d_staging) return AGT_ERR_ARG;
            e = hipMemcpyAsync(d_staging, h_frame, (size_t)src_w * src_h * 3, hipMemcpyHostToDevice, c->stream);
            if (e != hipSuccess) return hip_fail(c, e);
        }
        int rc = agt_preprocess_bgr(c, src, (size_t)src_w * 3, (size_t)src_w * src_h * 3, src_w, src_h, 1, undistort, roi_x, roi_y, W, H,
                                    d_gray, gpitch, gpitch * (size_t)H);
        if (rc) return rc;
    }
    AGT_TQ(1);
    int rc = AGT_OK;
    unsigned long long want = 0;
    if (polled) c->host_seq_on = 1;            // (every pose launch issued from here on reports the frames it solves)
    if (!registered) rc = agt_track_frame(c, d_gray, gpitch, gpitch * (size_t)H, 1, d_rec);
    if (polled && rc == AGT_OK) { want = c->hseq_off + (unsigned long long)c->trk_frame; c->hseq_last = want; }
    if (rc == AGT_OK) { AGT_TQ(2); rc = join_pipeline(c); }
    c->host_seq_on = 0;
    if (rc) return rc;
    AGT_TQ(3);
    if (polled) {
        if (d_state) {          // the device copy of the record, for callers that keep one (stream-ordered; nobody waits for it here)
            e = hipMemcpyAsync(d_state, c->hrec_dev, AGT_STATE_STRIDE * sizeof(double), hipMemcpyDeviceToDevice, c->stream);
            if (e != hipSuccess) return hip_fail(c, e);
        }
        AGT_TQ(4);
        rc = poll_seq(c, c->hseq_host, want);
        if (rc) return rc;
    } else {
        // (the waited form: profiling spans armed.  HSA_ENABLE_SDMA=0 -- blit-kernel copies -- made
        // the copy-first form of round 3 slower still: 107 us.)
        e = d_state ? hipMemcpyAsync(h_state, d_state, AGT_STATE_STRIDE * sizeof(double), hipMemcpyDeviceToHost, c->stream) : hipSuccess;
        AGT_TQ(4);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) return hip_fail(c, e);
    }
    // (unless a device record was read back: the record is in the context's host-mapped memory once the sequence word / the stream says so)
    if (polled || !d_state) memcpy(h_state, c->hrec_host, AGT_STATE_STRIDE * sizeof(double));
#ifdef AGT_DEBUG_KNOBS
    if (timing) { const double t5 = now(); for (int i = 0; i < 4; i++) acc.t[i] += tq[i + 1] - tq[i]; acc.t[4] += t5 - tq[4]; acc.t[5] += t5 - tq[0]; acc.n++; }
#endif
    return *(volatile int*)c->fault_host ? AGT_ERR_CHAIN : AGT_OK;
}
