"""The output stage on the device (include/agt_draw.h -> libagt_draw.so): display lists painted into frames that live in HBM, and the
reference's two images of a pose -- a dot on every projected model corner, the tag outlines on a black frame (detect_pose.py:441-465,
draw.py:63-153) -- built from projected points without the pose coming back to the host.

Drawing is binary and follows the integer rule of the header (discs  dx^2 + dy^2 <= r^2 + r,  segments = the pixels within T / 2 with
round caps); cv.LINE_AA and cv2's exact rasters are not reproduced.  Everything here enqueues on the current stream and returns
without synchronising.
"""
import numpy as np
import torch

from . import _sidelib
from . import drawlib as D
from .cv_hip import _raw_stream, _require_gpu

DOT_COLOR = (0, 0, 255)             # draw.py:151
LINE_COLOR = (255, 255, 255)        # draw.py:103-118
PRIM_BYTES = D.PRIM_DTYPE.itemsize


def prims_tensor(prims, device):
    """a host display list (drawlib.PRIM_DTYPE array [P] or [B, P], e.g. from drawlib.prims) -> cuda u8 [B, P, 32]"""
    a = np.ascontiguousarray(np.asarray(prims, D.PRIM_DTYPE))
    a = a.reshape((1, -1) if a.ndim < 2 else a.shape)
    return torch.from_numpy(a.view(np.uint8).reshape(a.shape[0], a.shape[1], PRIM_BYTES).copy()).to(device)


def prims_numpy(prims):
    """cuda u8 [B, P, 32] (or its numpy copy) -> structured array [B, P] with the fields of agt_draw_prim (synchronises)"""
    return _sidelib.records_numpy(prims, D.PRIM_DTYPE)


def draw_primitives(frames, prims, clear=False):
    """frames: cuda u8 [B, H, W] or [B, H, W, 3] with unit channel stride (3 channels: pixel stride 3); views with a row pitch and a
    frame stride are taken as they are.  prims: cuda u8 [B, P, 32] (agt_draw_prim records, contiguous; P may be 0).  The primitives of
    entry b are painted into frame b in list order, in place; clear=True also writes 0 to every pixel that none covers."""
    _require_gpu()
    assert frames.dtype == torch.uint8 and frames.is_cuda and frames.dim() in (3, 4), "frames must be cuda u8 [B, H, W] or [B, H, W, 3]"
    channels = 1 if frames.dim() == 3 else frames.shape[3]
    assert channels in (1, 3), "frames have 1 or 3 channels"
    if frames.dim() == 4:
        assert frames.stride(3) == 1 and frames.stride(2) == 3, "a colour frame is interleaved: channel stride 1, pixel stride 3"
    else:
        assert frames.stride(2) == 1, "a gray frame has unit pixel stride"
    B, h, w = frames.shape[:3]
    assert prims.dtype == torch.uint8 and prims.is_cuda and prims.is_contiguous() and prims.dim() == 3
    assert prims.shape[0] == B and prims.shape[2] == PRIM_BYTES and prims.device == frames.device
    P = prims.shape[1]
    dev = frames.device
    with torch.cuda.device(dev):
        args = _sidelib.frame_args(frames)
        D.raster(*args[:-1], channels, args[-1], prims.data_ptr() if P else None, P, D.CLEAR if clear else 0)
    return frames


def pose_lists(points, size, ok=None, radius=5, thickness=5, dot_color=DOT_COLOR, line_color=LINE_COLOR, corners_per_tag=4):
    """points: cuda f32 or f64 [B, n, 2] (contiguous; n a multiple of 4), size: (width, height) of the frames to be drawn into,
    ok: None or a cuda f64 tensor whose element [b * stride] gates entry b -- a column of state records, e.g. state[:, ST_OK] -- drawn
    where it is exactly 1.0.  -> (dots, outline), cuda u8 [B, n, 32] each: the discs of the overlay and the segments of the drawing
    frame (include/agt_draw.h states the rounding and the in-frame rule)."""
    _require_gpu()
    assert points.is_cuda and points.is_contiguous() and points.dim() == 3 and points.shape[2] == 2
    assert points.dtype in (torch.float32, torch.float64)
    B, n = points.shape[:2]
    width, height = int(size[0]), int(size[1])
    gate_ptr, gate_stride = None, 0
    if ok is not None:
        assert ok.is_cuda and ok.dtype == torch.float64 and ok.dim() == 1 and ok.shape[0] == B and ok.device == points.device
        gate_ptr, gate_stride = ok.data_ptr(), (ok.stride(0) if B > 1 else 1)
        assert gate_stride >= 1
    dev = points.device
    dots = torch.empty((B, n, PRIM_BYTES), dtype=torch.uint8, device=dev)
    outline = torch.empty((B, n, PRIM_BYTES), dtype=torch.uint8, device=dev)
    with torch.cuda.device(dev):
        D.pose_lists(_raw_stream(dev.index), points.data_ptr(), D.F32 if points.dtype == torch.float32 else D.F64, n, B, gate_ptr, gate_stride,
                     width, height, corners_per_tag, int(radius), int(thickness), D.pack_color(dot_color), D.pack_color(line_color),
                     dots.data_ptr(), outline.data_ptr())
    return dots, outline


def draw_pose(frames, draw_frames, points, ok=None, radius=5, thickness=5, dot_color=DOT_COLOR, line_color=LINE_COLOR):
    """The reference's two images of a pose: a dot of `radius` on every projected point that lies in the frame, painted into `frames`,
    and the outline of every tag that lies in the frame whole, `thickness` wide, on `draw_frames`, which is cleared first.  frames,
    draw_frames: as in draw_primitives, of one size; points, ok: as in pose_lists.  An entry whose gate is not 1.0 leaves its frame
    untouched and its drawing frame black.  -> (dots, outline)"""
    assert tuple(frames.shape[:3]) == tuple(draw_frames.shape[:3]), "frames and draw_frames are of one size and batch"
    dots, outline = pose_lists(points, (frames.shape[2], frames.shape[1]), ok, radius, thickness, dot_color, line_color)
    draw_primitives(frames, dots)
    draw_primitives(draw_frames, outline, clear=True)
    return dots, outline
