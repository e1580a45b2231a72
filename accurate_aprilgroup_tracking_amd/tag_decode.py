"""Tag payload decoding on the device (include/agt_tagcode.h -> libagt_tagcode.so): which tag does a quad show, how sure, or none.

The decode stage of a tag detector, applied to quads that something else found: the tracker's own corner buffer
(StreamTracker.decode_tags), the quad finder's candidates (tag_detect.detect_tags) or an outside detector's (cv_hip.decodeTags).
Finding quads in an image is quad_detect's job.  The margin is this rule's own scale (for a clean tag: half the local black / white contrast in gray levels), not
the decision_margin of any apriltag release.

A family is a list of 36-bit code words (bit 35 - (6 r + c) = row r, column c of the payload).  The real tag36h11 table is not
shipped: export it once from your own apriltag install with formats.save_tag_family.
"""
import collections

import numpy as np
import torch

from . import _sidelib
from . import tagcodelib as T
from .cv_hip import _raw_stream, _require_gpu

Decoded = collections.namedtuple("Decoded", "records ok corner_mask homography")
Decoded.__doc__ = """decode_quads' result, all cuda tensors: records u8 [B, Q, 40] (records_numpy gives the fields), ok u8 [B, Q],
corner_mask u8 [B, 4Q] (each verdict four times: the mask of StreamTracker.step_detected / estimate_pose), homography f64 [B, Q, 3, 3]
(square (+-1, +-1) -> the quad as given, not normalised)"""


class TagFamily:
    """codes: n <= 16384 words of a 6 x 6 family; name: what Detection.tag_family carries.  Host data; the device copy (the codes'
    four rotations) is made on first use, once per device and stream."""

    def __init__(self, codes, name="tag36", bits_per_side=6):
        self.codes = np.ascontiguousarray(np.asarray(codes, np.uint64).reshape(-1))
        self.name = name.decode() if isinstance(name, bytes) else str(name)
        self.bits_per_side = int(bits_per_side)
        if self.bits_per_side != 6:
            raise ValueError("TagFamily: only 6 x 6 payloads (bits_per_side = 6) are decoded")
        if not 1 <= self.codes.size <= T.MAX_CODES or np.any(self.codes >> np.uint64(36)):
            raise ValueError("TagFamily: 1..%d codes of at most 36 bits" % T.MAX_CODES)
        self._handles = {}

    def __len__(self):
        return self.codes.size

    def bits(self, ids=None):
        """(len(ids), 6, 6) u8 payloads of the given codes (all by default): what synthetic.render_frame paints"""
        codes = self.codes if ids is None else self.codes[np.asarray(ids, np.int64)]
        shifts = np.uint64(35) - np.arange(36, dtype=np.uint64)
        return ((codes[:, None] >> shifts[None, :]) & np.uint64(1)).astype(np.uint8).reshape(-1, 6, 6)

    def handle(self, device):
        """the tagcodelib.Family of torch's current stream on `device`"""
        key = (device, _raw_stream(device))
        if key not in self._handles:
            with torch.cuda.device(device):
                self._handles[key] = T.Family(self.codes, self.bits_per_side, key[1])
        return self._handles[key]


def decode_quads(frames, quads, family, mask=None, expected=None, max_hamming=2, min_margin=0.0):
    """frames: cuda u8 [B, H, W] (unit pixel stride; any row and frame stride), quads: cuda f32 [B, Q, 4, 2] in the model's corner order,
    mask: cuda u8 [B, Q] or None, expected: cuda i32 [Q] or None (then a verdict also needs id == expected[q] and rot == 0).
    Enqueues on the current stream and returns a Decoded without synchronising."""
    _require_gpu()
    assert _sidelib.is_gray_frames(frames), _sidelib.GRAY_FRAMES
    B, h, w = frames.shape
    assert quads.dtype == torch.float32 and quads.is_cuda and quads.is_contiguous() and quads.dim() == 4 and quads.shape[0] == B and tuple(quads.shape[2:]) == (4, 2)
    Q = quads.shape[1]
    if mask is not None:
        assert mask.dtype == torch.uint8 and mask.is_cuda and mask.is_contiguous() and tuple(mask.shape) == (B, Q)
    if expected is not None:
        assert expected.dtype == torch.int32 and expected.is_cuda and expected.is_contiguous() and tuple(expected.shape) == (Q,)
    dev = frames.device
    out = _outputs(B, Q, dev)
    # (the family's handle carries the stream)
    family.handle(dev.index).decode(*_sidelib.frame_args(frames)[1:], quads.data_ptr(), None if mask is None else mask.data_ptr(), Q,
                                    None if expected is None else expected.data_ptr(), max_hamming, min_margin, *[t.data_ptr() for t in out])
    return out


def _outputs(B, Q, dev):
    return Decoded(torch.empty((B, Q, T.RECORD_DTYPE.itemsize), dtype=torch.uint8, device=dev), torch.empty((B, Q), dtype=torch.uint8, device=dev),
                   torch.empty((B, 4 * Q), dtype=torch.uint8, device=dev), torch.empty((B, Q, 3, 3), dtype=torch.float64, device=dev))


def records_numpy(records):
    """records tensor (or its numpy copy) -> structured array [B, Q] with the fields of agt_tag_record (synchronises)"""
    return _sidelib.records_numpy(records, T.RECORD_DTYPE)


_TURN = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])     # square corner j -> corner j - 1


def records_to_detections(records, quads, homography, family_name="tag36"):
    """One batch entry's records [Q] (structured), quads [Q, 4, 2] and homographies [Q, 3, 3] on the host -> list of
    formats.Detection for the quads with status OK: corners rolled to the tag's canonical order (rot undone), homography mapping the
    canonical square onto them (normalised to H[2][2] = 1), center = H(0, 0), decision_margin = the record's margin."""
    from . import formats
    name = family_name.encode() if isinstance(family_name, str) else family_name
    out = []
    for rec, quad, Hq in zip(records, np.asarray(quads, np.float64), np.asarray(homography, np.float64)):
        if rec["status"] != T.TAG_OK:
            continue
        k = int(rec["rot"])
        Hc = Hq @ np.linalg.matrix_power(_TURN, k)
        Hc = Hc / Hc[2, 2]
        out.append(formats.make_detection(int(rec["id"]), np.roll(quad, k, axis=0), decision_margin=float(rec["margin"]), tag_family=name,
                                          hamming=int(rec["hamming"]), homography=Hc, center=Hc[:2, 2]))
    return out
