"""bench_c5.py -- BASELINE.json configs[4] for bench.py --workload c5: one 1280x720 stream, 60 tags / 240 corners,
LK + iterative PnP + dense photometric refinement (60 x 32 x 32 = 61,440 model samples) per frame.

A step = agt_track_frame_dense for one frame: pyrDown -> LK(240) -> solvePnP(240, guess) + gate + motion model -> `iters`
damped Gauss-Newton iterations over the 61,440 samples + 240 corners -> corner re-seed from the refined pose; stage kernels in
stream order, nothing leaves the device.  The kernel under the roofline is the dense accumulate (the "large-N Jacobian
reduce"): per launch M * 16 B of model (xyz f32 x 3 + template f32) + 12 one-byte taps per sample ("M * (12 + 4)
B model reads + gathered image taps").
"""
import json
import time

import numpy as np

ITERS, PHOTO_WEIGHT = 5, 0.05


def main_c5(args, torch, D, HL, wl, rank, world, dev, rehearsal):
    import bench as B_
    from accurate_aprilgroup_tracking_amd import synthetic as syn
    bench = B_.Bench(torch, wl, args, rank, world, dev)
    B, K, Wm, NPTS = bench.B, bench.K, bench.Wm, bench.npts
    sq = bench.seqs[0]
    mx = syn.model_samples(sq.group, 32)
    M = mx.shape[0]
    # template intensities: captured from the first frame at its known pose (the "model acquisition" step)
    T = np.nan_to_num(syn.sample_bilinear(sq.frame(0), syn.project(mx, sq.rvecs[0], sq.tvecs[0], sq.K)), nan=128.0).astype(np.float32)
    mxg, Tg = torch.from_numpy(mx).to(dev), torch.from_numpy(T).to(dev)
    trk = bench.trk
    trk.pipeline(0)
    trk.dense_model(mxg, Tg, iters=ITERS, photo_weight=PHOTO_WEIGHT, reseed=True)
    dense = torch.zeros((max(K, Wm, 1), B, HL.DENSE_STRIDE), dtype=torch.float64, device=dev)

    def run(n, out):
        # consecutive ring entries go to the tracker as one clip (agt_track_frames_dense: the same n steps and records as n calls of
        # step_dense; knowing the next frame, the library builds its pyramid inside the current frame's dense launch)
        k = 0
        while k < n:
            a = (bench.pos + 1) % bench.ring_slots
            m = min(n - k, bench.ring_slots - a, dense.shape[0] - (k % dense.shape[0])) if bench.clips else 1
            d0 = k % dense.shape[0]
            if m > 1:
                trk.step_many_dense(bench.ring[a:a + m], out[k:k + m] if out is not None else None, dense[d0:d0 + m])
            else:
                m = 1
                trk.step_dense(bench.ring[a], out[k] if out is not None else None, dense[d0])
            bench.pos += m; k += m
    bench.run = run                 # no detector refresh: the re-seed from the refined pose is the drift control here
    dts, st_warm, st_first, st_last, gathered = bench.timed_blocks(D, max(1, args.blocks), settle=not args.full)
    med, p10, p90 = B_.percentiles(dts)
    fps = world * B * K / med
    dn = dense.cpu().numpy()[:K]
    accepted = float(st_last[:, :, HL.ST_OK].mean())
    if rank == 0 and args.dump_outputs:
        # what the caller received for the last timed step: the state records of every rank, this rank's dense records
        B_.dump_outputs(args.dump_outputs, {"records": gathered[:, K - 1].cpu().numpy(), "dense_records": dn[K - 1]})
    if args.full:
        # accuracy against the generator's truth: PnP pose vs refined pose, last block
        err_pnp, err_ref = [], []
        for k in range(K):
            i = B_.pingpong(bench.pos - K + 1 + k, bench.NF)
            tr = np.concatenate([sq.rvecs[i], sq.tvecs[i]])
            err_pnp.append(np.abs(st_last[k, 0, :6] - tr).max()); err_ref.append(np.abs(dn[k, 0, :6] - tr).max())
    roof = cpu = None
    if rank == 0 and args.full:
        # per-kernel spans of an instrumented pass (HIP events on the launch stream, recorded by the library)
        Mf = min(K, 100)
        bench.restart()
        run(Wm, None)
        HL.check(trk.ctx.L.agt_profile_begin(trk.ctx.h, Mf), "agt_profile_begin")
        run(Mf, None)
        import ctypes as C
        ms = np.zeros((Mf, HL.PROF_SPANS), np.float32); nrec = C.c_int(0)
        HL.check(trk.ctx.L.agt_profile_end(trk.ctx.h, ms.ctypes.data_as(C.c_void_p), C.byref(nrec)), "agt_profile_end")
        spans = ms[:nrec.value].mean(axis=0) * 1e3
        accum_us = float(spans[3]) / ITERS
        bytes_per_launch = M * 16 + M * 12
        achieved = bytes_per_launch / (accum_us * 1e-6) / 1e9
        roof = {"bound": "hbm", "kernel": "dense_accum_kernel (61,440 samples: FP64 projection + 2x6 Jacobian, 12 image taps, 29 block-reduced sums)",
                "achieved": round(achieved, 3), "peak": B_.HBM_PEAK_GBS, "unit": "GB/s", "frac": round(achieved / B_.HBM_PEAK_GBS, 6),
                "traffic": B_.pmc_traffic("dense_accum_kernel"), "avg_launch_us": round(accum_us, 3), "launches_per_frame": ITERS,
                "bytes_per_launch": int(bytes_per_launch),
                "note": "latency-bound: one stream, 240 blocks, a dependent FP64 chain per sample; the image taps come from L2",
                "stage_spans_us": {"pyramid": round(float(spans[0]), 2), "lk(240)": round(float(spans[1]), 2), "pnp(240)": round(float(spans[2]), 2),
                                   "dense_gauss_newton(x%d launches)" % ITERS: round(float(spans[3]), 2), "dense_final(update+reseed)": round(float(spans[4]), 2)},
                "stage_spans_note": "instrumented pass: every stage a launch of its own (HIP events between them); the timed blocks run LK | PnP as one "
                                    "chained launch with the previous frame's final step as the LK prologue, so their frame is shorter than the sum of these spans"}
        if not args.no_cpu_baseline and world == 1:
            cpu = cpu_baseline_c5(sq, bench.rendered[:, 0], mx, T, bench.NF)
    if rank == 0:
        out = {"metric": "frames/sec (LK+PnP+dense refinement) on 1280x720 60-tag stream", "value": round(fps, 2), "unit": "frames/s",
               "n_gpus": world, "steps": K, "warmup": Wm, "ms_per_step": round(med / K * 1e3, 5),
               "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "u8/i64 (LK), f64 (PnP, dense GN)",
               "data": "synthetic",
               "config": {"workload": wl["label"] % B, "streams_per_gpu": B, "dense_samples": M, "gn_iterations": ITERS, "photo_weight": PHOTO_WEIGHT,
                          "corner_reseed": True, "launch": ("frames handed over as clips (agt_track_frames_dense): %d launches per frame -- one chained launch [previous frame's last Gauss-Newton update + corner re-seed as the LK workgroups' prologue | LK | four-wave PnP behind the arrival count | the next frame's pyramid pass], then the %d accumulate launches" % (1 + ITERS, ITERS)) if bench.clips else ("stage kernels in stream order, one call per frame (%d launches per frame)" % (3 + ITERS + 1))},
               "timing": {"blocks": len(dts), "steps_per_block": K, "statistic": B_.block_statistic(dts),
                          "ms_per_step_p10": round(p10 / K * 1e3, 5), "ms_per_step_p90": round(p90 / K * 1e3, 5)},
               "roofline": roof, "cpu_baseline": cpu, "accepted_frac": round(accepted, 4),
               "refined_frac": round(float(dn[:, :, HL.DN_REFINED].mean()), 4), "tracked_corners_mean": round(float(st_last[:, :, HL.ST_NTRACK].mean()), 1),
               "max_abs_pose_err_vs_truth": {"pnp": float(np.max(err_pnp)), "dense_refined": float(np.max(err_ref))} if args.full else None,
               "render_s": round(bench.render_s, 1), "gathered_shape": list(gathered.shape), "rccl_ranks": world, "dist_backend": D.backend_name()}
        if rehearsal:
            out["rehearsal"] = True
        print(json.dumps(out), flush=True)
    D.barrier()


def cpu_baseline_c5(seq, frames, mx, T, NF):
    """the same chain on ONE host core with the oracle ("port"), ~10 s: cvo_track_frame (pyramid + Scharr + LK + LM over 240
    corners) + dense_refine (61,440 samples, 5 GN iterations) + re-seed"""
    import bench as B_
    cvo, flags = B_.native_oracle()
    pyr = cvo.Pyramid(frames[0]); pts = seq.corners(0)
    r, t = seq.rvecs[0].copy(), seq.tvecs[0].copy()
    n = 0; t0 = time.perf_counter()
    while True:
        k = B_.pingpong(n + 1, NF)
        pyr, pts, stt, er, cnt, r, t = cvo.track_frame(pyr, frames[k], pts, seq.obj, seq.K, None, r, t, nthreads=1)
        r, t, _ = cvo.dense_refine(frames[k], mx, T, seq.obj, pts, stt, seq.K, None, r, t, iters=ITERS, photo_weight=PHOTO_WEIGHT)
        pp, _ = cvo.projectPoints(seq.obj, r, t, seq.K, None)
        pts = pp.reshape(-1, 2).astype(np.float32)
        n += 1
        if time.perf_counter() - t0 > 10.0:
            break
    dt = time.perf_counter() - t0
    import os
    return {"value": round(n / dt, 2), "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": "%d frames of the same stream: oracle cvo_track_frame (240 corners) + dense_refine (%d samples, %d GN iterations) + re-seed, "
                      "1 thread, %.1f s; host has %d cores" % (n, mx.shape[0], ITERS, dt, os.cpu_count()),
            "cpu_model": B_.cpu_model(), "build": flags}
