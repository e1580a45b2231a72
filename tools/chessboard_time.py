"""Cost of the chessboard corner finder (include/agt_chess.h) on the device: microseconds per agt_chess_corners call on rendered boards
(tests/chess_scenes.py), by HIP events around blocks of calls (outputs allocated once by the first call and the allocator's cache), the
median over the blocks; then one find_chessboard call with its host assembly by the host clock.
--once runs each shape a few times without timing, for a profiler's kernel trace (rocprofv3 --kernel-trace --stats -- python ... --once).

    python tools/chessboard_time.py [--calls 200] [--blocks 21] [--once]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

SHAPES = [("e2e", 1), ("e2e", 16), ("cam5", 1)]           # 1280x720 at B = 1 and 16, 640x480 at B = 1


def traffic_bytes(w, h, candidates, max_candidates, half):
    """bytes the kernels must move per frame, counted from the shapes: the frame read once and the 4-byte response written by
    ch_response, the response read and the byte mask written by ch_count, the mask read by ch_emit, the table and the records; the
    suppression windows and the refinement's samples fall into lines already fetched and are not counted"""
    n = w * h
    phases = {"response": n + 4 * n, "count": 4 * n + n, "scan": 12 * max_candidates, "emit": n + 12 * candidates,
              "refine": candidates * (2 * half + 4) ** 2 + 48 * max_candidates}
    return phases, sum(phases.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    import chess_scenes as S
    from accurate_aprilgroup_tracking_amd import chessboard
    assert torch.cuda.is_available(), "needs a GPU"
    out = []
    for name, B in SHAPES:
        views = S.class_views(name, True)
        frames = torch.from_numpy(np.stack([views[k % len(views)][0] for k in range(B)])).cuda()
        w, h = S.CLASSES[name][1]
        fd = chessboard.ChessboardFinder(w, h, B)
        res = fd.corners(frames)
        torch.cuda.synchronize()
        counts = res.counts.cpu().numpy()
        if a.once:
            for _ in range(5):
                fd.corners(frames)
            torch.cuda.synchronize()
            continue
        for _ in range(a.warmup):
            fd.corners(frames)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                fd.corners(frames)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        t = []
        for _ in range(5):
            t0 = time.perf_counter()
            found = chessboard.find_chessboard(frames, S.PATTERN, fd)
            t.append(time.perf_counter() - t0)
        phases, total = traffic_bytes(w, h, int(counts[0, 1]), fd.max_candidates, 5)
        row = dict(scene=name, width=w, height=h, B=B, counts_frame0=counts[0].tolist(), us_per_call=float(np.median(us)), us_min=float(min(us)),
                   us_max=float(max(us)), us_per_frame=float(np.median(us)) / B, found=[bool(f) for f, _ in found],
                   find_chessboard_ms=1000.0 * float(np.median(t)), bytes_per_frame=total, bytes_over_frame=total / float(w * h), phases=phases)
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


if __name__ == "__main__":
    main()
