"""Finding tag quads on the device (include/agt_quadfind.h -> libagt_quadfind.so): "a quad is roughly here", with no seed.

The first stage of a tag detector: the frame is thresholded against its local contrast, the dark pixels are labelled into 4-connected
components and every component whose outline is close to a convex quadrilateral becomes a candidate.  The rule is integer only, so
the result is the same bits on every run.  It delivers recall and corners within a few pixels; quad_refine.refine_quads gives the
accuracy and tag_decode.decode_quads refuses what is no tag (tag_detect.detect_tags runs the three in a row).
Limits: 4-connectivity; a quiet zone under about 2 px merges a tag with its surroundings.
"""
import collections

import torch

from . import _sidelib
from . import quadfindlib as Q
from .cv_hip import _require_gpu

Found = collections.namedtuple("Found", "quads records counts")
Found.__doc__ = """QuadDetector.detect's result, all cuda tensors: quads f32 [B, max_quads, 4, 2] (contiguous: quad_refine.refine_quads
and tag_decode.decode_quads take it as it is; the vertices run clockwise on the screen), records u8 [B, max_quads, 32] (records_numpy
gives the fields: label, area, x0, y0, x1, y1, s2), counts i32 [B, 4]: dark components, components inside the area limits, candidates
before the max_quads cap, flag bits (quadfindlib.FLAG_QUADS, FLAG_COMPONENTS).  The first min(counts[b, 2], max_quads) entries of frame
b are candidates in ascending label order; the rest are zero."""


def _check_frames(frames, width, height, max_batch):
    return _sidelib.check_frames(frames, Q.MIN_SIZE, width, height, max_batch, Q.QuadFindError, "QuadDetector")


class QuadDetector:
    """The workspace of the quad finder for frames of up to width x height in batches of up to max_batch.  Frames of any size from
    8 x 8 up to that are accepted per call.  max_components: the components inside the area limits that are examined per frame;
    max_quads: the candidates written per frame.  Calls on one QuadDetector share the workspace: issue them on one stream."""

    def __init__(self, width, height, max_batch=1, max_components=4096, max_quads=512):
        self.width, self.height, self.max_batch = int(width), int(height), int(max_batch)
        self.max_components, self.max_quads = int(max_components), int(max_quads)
        for name, v, lo, hi in (("width", self.width, Q.MIN_SIZE, Q.MAX_SIZE), ("height", self.height, Q.MIN_SIZE, Q.MAX_SIZE),
                                ("max_batch", self.max_batch, 1, Q.MAX_BATCH), ("max_components", self.max_components, 1, Q.MAX_COMPONENTS),
                                ("max_quads", self.max_quads, 1, self.max_components)):
            if not lo <= v <= hi:
                raise Q.QuadFindError(Q.ERR_ARG, "QuadDetector(%s=%d), limits %d..%d" % (name, v, lo, hi))
        self._finder = _sidelib.PerDevice(Q.Finder, self.width, self.height, self.max_batch, self.max_components, self.max_quads)

    def detect(self, frames, **options):
        """frames: cuda u8 [B, H, W] (unit pixel stride; any row and frame stride).  options: min_contrast (40), min_area (24),
        max_area (INT32_MAX), min_fill_pct (5).  Enqueues on the current stream and returns a Found without synchronising."""
        opts = Q.options(**options)
        B, h, w = _check_frames(frames, self.width, self.height, self.max_batch)
        _require_gpu()
        dev = frames.device
        out = Found(torch.empty((B, self.max_quads, 4, 2), dtype=torch.float32, device=dev),
                    torch.empty((B, self.max_quads, Q.RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev),
                    torch.empty((B, 4), dtype=torch.int32, device=dev))
        self.detect_into(frames, out, opts)
        return out

    def detect_into(self, frames, out, opts=None):
        """detect() into the tensors of `out` (a Found, or any three cuda tensors of those shapes with 4-byte aligned storage)"""
        _check_frames(frames, self.width, self.height, self.max_batch)
        dev = frames.device
        with torch.cuda.device(dev):
            self._finder(dev.index).detect(*_sidelib.frame_args(frames), opts, *[t.data_ptr() for t in out])
        return out

    def labels(self, frames, min_contrast=40):
        """-> cuda i32 [B, H, W]: the smallest linear index y * W + x of each dark pixel's 4-connected component, -1 elsewhere"""
        B, h, w = _check_frames(frames, self.width, self.height, self.max_batch)
        _require_gpu()
        dev = frames.device
        out = torch.empty((B, h, w), dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            self._finder(dev.index).labels(*_sidelib.frame_args(frames), min_contrast, out.data_ptr())
        return out


def records_numpy(records):
    """records tensor (or its numpy copy) -> structured array [B, max_quads] with the fields of agt_quadfind_record (synchronises)"""
    return _sidelib.records_numpy(records, Q.RECORD_DTYPE)
