"""Edge refinement of tag quads on the device (include/agt_quadfit.h -> libagt_quadfit.so): a roughly known quad snapped onto the
tag's border, or refused.

The stage of a tag detector between "a quad is roughly here" and "decode it": a line is fitted to the black-to-white step along each
of the four border edges and the lines are intersected.  The seeds come from something else: the tracker's own corner buffer
(StreamTracker.refine_tags), re-projected corners, the quad finder's candidates (tag_detect.detect_tags) or an outside detector's
(cv_hip.refineQuads).  Finding quads without a seed is quad_detect's job.  The strength of a record is the mean step height along the weakest edge in gray levels: above
100 on a tag's border, around 10 on background texture.
"""
import collections

import torch

from . import _sidelib
from . import quadfitlib as Q
from .cv_hip import _require_gpu

Refined = collections.namedtuple("Refined", "quads quads64 records ok corner_mask")
Refined.__doc__ = """refine_quads' result, all cuda tensors: quads f32 [B, Q, 4, 2] (contiguous: tag_decode.decode_quads takes it as
it is) and quads64 f64 [B, Q, 4, 2] -- the refined corners where ok, the input corners bit for bit elsewhere --, records u8 [B, Q, 32]
(records_numpy gives the fields), ok u8 [B, Q], corner_mask u8 [B, 4Q] (each verdict four times: the mask of
StreamTracker.step_detected / estimate_pose)"""


def refine_quads(frames, quads, mask=None, range_px=2.0, iters=2, min_strength=40.0):
    """frames: cuda u8 [B, H, W] (unit pixel stride; any row and frame stride), quads: cuda f32 [B, Q, 4, 2] on the outer edge of the
    black border, either orientation, mask: cuda u8 [B, Q] or None.  range_px: how far along its normal an edge is searched (at most
    an eighth of the edge's length); a quad that moves further than 2 range_px is refused.  iters: passes, 1..8.  min_strength: the
    weakest edge's mean step height a quad needs.  Enqueues on the current stream and returns a Refined without synchronising."""
    _require_gpu()
    assert _sidelib.is_gray_frames(frames), _sidelib.GRAY_FRAMES
    B, h, w = frames.shape
    assert quads.dtype == torch.float32 and quads.is_cuda and quads.is_contiguous() and quads.dim() == 4 and quads.shape[0] == B and tuple(quads.shape[2:]) == (4, 2)
    nq = quads.shape[1]
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and tuple(mask.shape) == (B, nq)
    dev = frames.device
    out = Refined(torch.empty((B, nq, 4, 2), dtype=torch.float32, device=dev), torch.empty((B, nq, 4, 2), dtype=torch.float64, device=dev),
                  torch.empty((B, nq, Q.RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev), torch.empty((B, nq), dtype=torch.uint8, device=dev),
                  torch.empty((B, 4 * nq), dtype=torch.uint8, device=dev))
    with torch.cuda.device(dev):
        Q.refine(*_sidelib.frame_args(frames), quads.data_ptr(), None if mask is None else mask.data_ptr(), nq, range_px, iters,
                 min_strength, *[t.data_ptr() for t in out])
    return out


def records_numpy(records):
    """records tensor (or its numpy copy) -> structured array [B, Q] with the fields of agt_quad_record (synchronises)"""
    return _sidelib.records_numpy(records, Q.RECORD_DTYPE)
