"""A tag detector with nothing from outside: find (quad_detect, include/agt_quadfind.h) -> refine (quad_refine, agt_quadfit.h) ->
decode (tag_decode, agt_tagcode.h), all on the device.

detect_tags is the chain on cuda tensors; DeviceTagDetector wraps it as the callable `detector(gray)` that PoseDetector takes in place
of the swatbotics apriltag module:

    family = formats.load_tag_family("tag36h11.npz")
    det = PoseDetector(logger, mtx, dist, enhance_ape, detector=DeviceTagDetector(family), backend="stream")
"""
import collections

import numpy as np
import torch

from . import quad_detect, quad_refine, tag_decode

Tags = collections.namedtuple("Tags", "quads ids rotations margins ok found refined decoded")
Tags.__doc__ = """detect_tags' result, all cuda tensors over the finder's candidate slots [B, max_quads]: quads f32 [B, Q, 4, 2] (the
refined corners where the quad was refined, the finder's elsewhere; in the finder's vertex order, NOT rolled), ids / rotations i32
[B, Q] (-1 where no payload was read; np.roll(quad, rot, axis=0) is the tag's own corner order), margins f64 [B, Q] (decode's scale),
ok u8 [B, Q]: 1 iff the candidate was refined and decoded to a tag of the family.  found / refined / decoded: the three stages' own
results (quad_detect.Found, quad_refine.Refined, tag_decode.Decoded); found.counts[b, 2] says how many slots of frame b were
candidates at all."""


def detect_tags(frames, family, detector=None, max_hamming=2, min_margin=0.0, range_px=2.0, iters=2, min_strength=40.0, **find_options):
    """frames: cuda u8 [B, H, W]; family: a tag_decode.TagFamily; detector: a quad_detect.QuadDetector to reuse (one is made for the
    call otherwise, which allocates); find_options: those of QuadDetector.detect.  The refinement's verdict is the decode's mask, so a
    slot past a frame's candidate count (a zero quad) is never decoded.  Enqueues on the current stream; no synchronisation."""
    if detector is None:
        B, h, w = quad_detect._check_frames(frames, quad_detect.Q.MAX_SIZE, quad_detect.Q.MAX_SIZE, quad_detect.Q.MAX_BATCH)
        detector = quad_detect.QuadDetector(w, h, max_batch=B)
    found = detector.detect(frames, **find_options)
    refined = quad_refine.refine_quads(frames, found.quads, range_px=range_px, iters=iters, min_strength=min_strength)
    decoded = tag_decode.decode_quads(frames, refined.quads, family, mask=refined.ok, max_hamming=max_hamming, min_margin=min_margin)
    words = decoded.records.view(torch.int32)                     # agt_tag_record: id, hamming, rot, status, then three 8-byte fields
    return Tags(refined.quads, words[..., 0], words[..., 2], decoded.records.view(torch.float64)[..., 2], decoded.ok, found, refined, decoded)


def corner_table(tags, lut, n_tags):
    """The candidates that decoded to a tag of the model, as the model's corner table, on the device.  lut: cuda i64 [len(family)],
    family index -> tag of the model or -1.  -> (corners f32 [B, 4 n_tags, 2], corner_mask u8 [B, 4 n_tags]): corners rolled by the
    decoded rotation into model order; of two candidates with one id the larger margin wins, on a tie the lower candidate index;
    every other tag's corners and mask bytes are 0."""
    B, Q = tags.ok.shape
    dev = tags.ok.device
    ids = tags.ids.to(torch.int64)
    tag = torch.where((tags.ok != 0) & (ids >= 0), lut[ids.clamp(0, lut.numel() - 1)], torch.full_like(ids, -1))
    valid = tag >= 0
    slot = torch.where(valid, tag, torch.full_like(tag, n_tags))                          # (a spare column takes the rest)
    margin = torch.where(valid, tags.margins, torch.full_like(tags.margins, -1.0))
    best = torch.full((B, n_tags + 1), -1.0, dtype=torch.float64, device=dev).scatter_reduce(1, slot, margin, "amax", include_self=True)
    index = torch.arange(Q, device=dev, dtype=torch.int64).expand(B, Q)
    wins = valid & (margin == best.gather(1, slot))
    first = torch.full((B, n_tags + 1), Q, dtype=torch.int64, device=dev).scatter_reduce(1, torch.where(wins, slot, torch.full_like(slot, n_tags)),
                                                                                           index, "amin", include_self=True)[:, :n_tags]
    have = first < Q
    pick = first.clamp(max=Q - 1)
    quads = tags.quads.gather(1, pick[:, :, None, None].expand(B, n_tags, 4, 2))
    rot = tags.rotations.to(torch.int64).gather(1, pick)
    order = (torch.arange(4, device=dev)[None, None, :] - rot[:, :, None]) % 4            # np.roll(quad, rot, axis=0)
    quads = quads.gather(2, order[:, :, :, None].expand(B, n_tags, 4, 2))
    corners = torch.where(have[:, :, None, None], quads, torch.zeros_like(quads)).reshape(B, 4 * n_tags, 2).contiguous()
    mask = have.to(torch.uint8)[:, :, None].expand(B, n_tags, 4).reshape(B, 4 * n_tags).contiguous()
    return corners, mask


def family_lut(family, tag_ids, n_tags, device):
    """tag_ids: the family index of each tag of the model in model order (None: 0..n_tags-1) -> cuda i64 [len(family)]"""
    ids = np.arange(n_tags, dtype=np.int64) if tag_ids is None else np.asarray(tag_ids, np.int64).reshape(-1)
    if ids.size != n_tags or len(set(ids.tolist())) != n_tags or ids.min() < 0 or ids.max() >= len(family):
        raise ValueError("tag_ids: one distinct family index (0..%d) per tag of the model" % (len(family) - 1))
    lut = np.full(len(family), -1, np.int64)
    lut[ids] = np.arange(n_tags)
    return torch.from_numpy(lut).to(device)


class DeviceTagDetector:
    """A callable `detector(gray)` for PoseDetector, group_calib and camera_calib in place of apriltag.Detector().detect: gray (H, W)
    u8 on the host -> list of formats.Detection (tag_id, corners (4, 2) in the tag's own corner order -- the one
    formats.detections_to_corner_table expects --, decision_margin, hamming, homography, center), in the finder's label order.
    decision_margin is tag_decode's OWN margin scale (about half the local black / white contrast in gray levels, near 100 for a
    tag printed 30 / 225), not the decision_margin of any apriltag release: thresholds do not carry over, though PoseDetector's cut
    at 50 happens to suit both.  min_margin: candidates below it are dropped here.  The workspace is kept per frame size."""

    def __init__(self, family, min_margin=0.0, max_hamming=2, max_components=4096, max_quads=512, **options):
        self.family, self.min_margin, self.max_hamming = family, float(min_margin), int(max_hamming)
        self.max_components, self.max_quads, self.options = int(max_components), int(max_quads), dict(options)
        quad_detect.Q.options(**{k: v for k, v in self.options.items() if k in quad_detect.Q.DEFAULTS})
        self._detectors = {}

    def __call__(self, gray):
        from .cv_hip import _require_gpu
        img = np.ascontiguousarray(np.asarray(gray))
        if img.dtype != np.uint8 or img.ndim != 2:
            raise ValueError("DeviceTagDetector: gray must be a 2-D uint8 image")
        _require_gpu()
        dev = torch.device("cuda", torch.cuda.current_device())
        key = (dev.index,) + img.shape
        if key not in self._detectors:
            self._detectors[key] = quad_detect.QuadDetector(img.shape[1], img.shape[0], 1, self.max_components, self.max_quads)
        tags = detect_tags(torch.from_numpy(img).to(dev)[None], self.family, detector=self._detectors[key], max_hamming=self.max_hamming,
                           min_margin=self.min_margin, **self.options)
        n = min(int(tags.found.counts[0, 2]), self.max_quads)
        return tag_decode.records_to_detections(tag_decode.records_numpy(tags.decoded.records)[0, :n], tags.quads.cpu().numpy()[0, :n],
                                                tags.decoded.homography.cpu().numpy()[0, :n], self.family.name)
