"""Cost of the quad finder (include/agt_quadfind.h) on the device: microseconds per agt_quadfind_detect call on the tests' scenes, by HIP
events around blocks of calls (outputs allocated once), the median over the blocks; --cpu adds the time of the numpy + scipy chain on
one core (scipy.ndimage.label for the labelling, the numpy statement of tests/quad_detect_numpy.py for the rest), a baseline only.
--once runs each shape a few times without timing, for a profiler's kernel trace (rocprofv3 --kernel-trace --stats -- python ... --once).

    python tools/quad_detect_time.py [--calls 200] [--blocks 21] [--cpu] [--once]
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

SHAPES = [("dense", 1), ("dense", 16), ("small", 1)]           # 1280x720 at B = 1 and 16, 640x480 at B = 1


def traffic_bytes(w, h, dark, kept, max_quads):
    """bytes the eleven kernels move per frame, counted from the shapes (n pixels, n / 16 tiles, `dark` dark pixels, `kept` components
    in the table): what each phase must read and write once.  A lower estimate: neighbour reads that fall into lines already fetched,
    the steps of the union-find walks and the atomics are not counted."""
    n, nt = w * h, (w // 4) * (h // 4)
    borders = ((w - 1) // 64) * h + ((h - 1) // 16) * w
    phases = {"tile_minmax": n + 2 * nt, "tile_neigh": 2 * nt + 2 * nt, "label_tiles": n + 2 * nt + 8 * n, "merge_borders": 8 * borders,
              "flatten_area": 4 * n + 8 * dark, "root_count": 4 * n, "root_assign": 4 * n + kept * (8 + 4 + 128), "support": 4 * n,
              "quads": kept * (128 + 4 + 4 + 32 + 32), "emit": kept * 4 + 2 * max_quads * 32}
    return phases, sum(phases.values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--blocks", type=int, default=21)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--cpu", action="store_true")
    ap.add_argument("--once", action="store_true")
    a = ap.parse_args()
    import torch
    import tag_decode_scenes as ts
    from accurate_aprilgroup_tracking_amd import quad_detect
    assert torch.cuda.is_available(), "needs a GPU"
    out = []
    for name, B in SHAPES:
        seq = ts.sequence(name)
        frames = torch.from_numpy(np.stack([seq.frame(k % 2) for k in range(B)])).cuda()
        det = quad_detect.QuadDetector(seq.width, seq.height, max_batch=B)
        res = det.detect(frames)
        torch.cuda.synchronize()
        counts = res.counts.cpu().numpy()
        if a.once:
            for _ in range(5):
                det.detect_into(frames, res)
            torch.cuda.synchronize()
            continue
        for _ in range(a.warmup):
            det.detect_into(frames, res)
        torch.cuda.synchronize()
        us = []
        for _ in range(a.blocks):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.calls):
                det.detect_into(frames, res)
            e1.record()
            e1.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / a.calls)
        lab = det.labels(frames[:1])
        torch.cuda.synchronize()
        dark = int((lab >= 0).sum())
        phases, total = traffic_bytes(seq.width, seq.height, dark, min(int(counts[0, 1]), det.max_components), det.max_quads)
        row = dict(scene=name, width=seq.width, height=seq.height, B=B, counts_frame0=counts[0].tolist(), us_per_call=float(np.median(us)),
                   us_min=float(min(us)), us_max=float(max(us)), us_per_frame=float(np.median(us)) / B, dark_pixels=dark,
                   bytes_per_frame=total, bytes_over_frame=total / float(seq.width * seq.height), phases=phases)
        if a.cpu and B == 1:
            import quad_detect_numpy as qd
            from scipy import ndimage
            img = seq.frame(0)
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                mask = qd.dark_mask(img)
                lab_s, n = ndimage.label(mask)
                index = np.arange(img.size).reshape(img.shape)
                smallest = np.asarray(ndimage.minimum(index, lab_s, np.arange(1, n + 1))).astype(np.int64)
                lab_n = np.where(lab_s > 0, np.concatenate([[-1], smallest])[lab_s], -1).astype(np.int32)
                qd.detect(img, lab=lab_n)
                t.append(time.perf_counter() - t0)
            row["numpy_scipy_ms"] = 1000.0 * float(np.median(t))
        out.append(row)
        print(json.dumps(row), flush=True)
    return out


if __name__ == "__main__":
    main()
