"""-m gpu: the quad finder (include/agt_quadfind.h) against the numpy statement of its rule (tests/quad_detect_numpy.py), byte for
byte -- labels, quads, records and counts; the rule has no float in it, so there is no tolerance and nothing is left out -- on the
patterns that break labelling kernels, the rendered scenes and single quads, at the caps, in batches and odd storage, at the options'
edges, and through its public doors (quad_detect.QuadDetector, tag_detect.detect_tags / DeviceTagDetector, cv_hip.detectQuads,
StreamTracker.detect_tags)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quad_detect_numpy as qd      # noqa: E402
import quad_detect_scenes as S      # noqa: E402
import tag_decode_scenes as ts      # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    torch.cuda.set_device(0)
    return torch


def device_detect(torch, frames, detector=None, max_components=4096, max_quads=512, **options):
    """host frames [B, H, W] (or a cuda tensor) -> (quads f32 [B, Q, 4, 2], records [B, Q] structured, counts i32 [B, 4]) on the host"""
    from accurate_aprilgroup_tracking_amd import quad_detect
    f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.array(frames)).cuda()
    if detector is None:
        detector = quad_detect.QuadDetector(f.shape[2], f.shape[1], f.shape[0], max_components, max_quads)
    out = detector.detect(f, **options)
    torch.cuda.synchronize()
    assert out.quads.is_contiguous() and out.quads.dtype == torch.float32 and tuple(out.quads.shape) == (f.shape[0], detector.max_quads, 4, 2)
    return out.quads.cpu().numpy(), quad_detect.records_numpy(out.records), out.counts.cpu().numpy()


def same_bytes(got, want, what=""):
    for name, g, w in zip(("quads", "records", "counts"), got, want):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint8).reshape(g.shape[0], -1) != w.view(np.uint8).reshape(w.shape[0], -1))[0]
            raise AssertionError("%s: %s differ, first at frame %d byte %d; device counts %s, numpy counts %s" %
                                 (what, name, bad[0], bad[1], got[2].tolist(), want[2].tolist()))


# ---- labels

@pytest.mark.parametrize("w,h", S.LABEL_SIZES + [(257, 129)])
def test_labels_on_patterns_that_break_labelling_kernels(torch_cuda, w, h):
    """spiral, comb, U, serpentine, blobs touching by a corner, one-pixel checkerboard, uniform: one batch per size"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import quad_detect
    frames, masks, want = S.pattern_frames(w, h)
    det = quad_detect.QuadDetector(w, h, max_batch=len(frames))
    got = det.labels(torch.from_numpy(np.array(frames)).cuda())
    torch.cuda.synchronize()
    assert got.dtype == torch.int32 and tuple(got.shape) == want.shape
    got = got.cpu().numpy()
    for p, g, l in zip(S.PATTERNS, got, want):
        assert np.array_equal(g >= 0, l >= 0), "%s: the dark mask" % p.__name__
        assert g.tobytes() == l.tobytes(), "%s: %d labels differ" % (p.__name__, int((g != l).sum()))
    # the same through detect: every dark component counted, the checkerboard's thousands of one-pixel components included
    counts = device_detect(torch, frames, detector=det, min_area=1)[2]
    assert counts[:, 0].tolist() == [len(np.unique(l[l >= 0])) for l in want]
    same_bytes(device_detect(torch, frames, detector=det, min_area=1), qd.detect_batch(frames, min_area=1), "patterns %dx%d" % (w, h))


@pytest.mark.parametrize("name,k", [("small", 0), ("dense", 0)])
def test_labels_on_scenes(torch_cuda, name, k):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import quad_detect
    img = ts.sequence(name).frame(k)
    got = quad_detect.QuadDetector(img.shape[1], img.shape[0]).labels(torch.from_numpy(img[None]).cuda())
    torch.cuda.synchronize()
    assert got.cpu().numpy()[0].tobytes() == qd.labels(img).tobytes()


# ---- detect

@pytest.mark.parametrize("name,k", [("small", 0), ("small", 1), ("c2", 0), ("dense", 0)])
def test_detect_on_scenes(torch_cuda, name, k):
    want = S.numpy_chain(name, k)
    got = device_detect(torch_cuda, ts.sequence(name).frame(k)[None])
    print(name, k, "counts", got[2][0].tolist())
    same_bytes(got, tuple(a[None] for a in (want["quads"], want["records"], want["counts"])), "%s %d" % (name, k))
    assert got[2][0, 3] == 0 and 0 < got[2][0, 2] < 512


@pytest.mark.parametrize("i", range(len(S.SINGLE_QUADS)))
def test_detect_on_single_quads(torch_cuda, i):
    frame, truth = S.single_quad(i)
    got = device_detect(torch_cuda, frame[None])
    same_bytes(got, qd.detect_batch(frame[None]), str(S.SINGLE_QUADS[i]))
    assert got[2][0, 2] == 1 and S.match_error(got[0][0, 0], truth)[0] <= 2.0


def test_detect_at_the_frame_borders(torch_cuda):
    """a quad with dark pixels in a border row or column is dropped, one 1.5 px inside is kept"""
    cases = S.border_quads()
    frames = np.stack([f for _, f, _ in cases])
    got = device_detect(torch_cuda, frames)
    same_bytes(got, qd.detect_batch(frames), "borders")
    assert got[2][:, 2].tolist() == [1 if kind == "inside" else 0 for kind, _, _ in cases]


# ---- caps, batches, storage

def test_caps_keep_the_first_in_label_order(torch_cuda):
    img = ts.sequence("small").frame(0)[None]
    full = device_detect(torch_cuda, img)
    n = int(full[2][0, 2])
    few = device_detect(torch_cuda, img, max_quads=5)
    same_bytes(few, qd.detect_batch(img, max_quads=5), "max_quads=5")
    assert few[2][0].tolist() == [full[2][0, 0], full[2][0, 1], n, qd.FLAG_QUADS] and few[1].tobytes() == full[1][:, :5].tobytes()
    cut = device_detect(torch_cuda, img, max_components=7, max_quads=7)
    same_bytes(cut, qd.detect_batch(img, max_components=7, max_quads=7), "max_components=7")
    m = int(cut[2][0, 2])
    assert cut[2][0, 3] == qd.FLAG_COMPONENTS and cut[2][0, 1] == full[2][0, 1] and m <= 7 and cut[1][0, :m].tobytes() == full[1][0, :m].tobytes()
    both = device_detect(torch_cuda, img, max_components=40, max_quads=5)
    same_bytes(both, qd.detect_batch(img, max_components=40, max_quads=5), "both caps")
    assert both[2][0, 3] == qd.FLAG_QUADS | qd.FLAG_COMPONENTS


def test_caps_leave_the_guard_bytes_alone(torch_cuda):
    """max_quads = 5 and max_components = 7 with 64 guard bytes in front of and behind every output"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import quad_detect
    img = torch.from_numpy(ts.sequence("small").frame(0)[None]).cuda()
    for maxc, maxq in ((4096, 5), (7, 5)):
        det = quad_detect.QuadDetector(640, 480, 1, maxc, maxq)
        sizes = [maxq * 32, maxq * 32, 16]
        bufs = [torch.full((n + 128,), 0xA5, dtype=torch.uint8, device="cuda") for n in sizes]
        out = (bufs[0][64:64 + sizes[0]].view(torch.float32).view(1, maxq, 4, 2), bufs[1][64:64 + sizes[1]].view(1, maxq, 32),
               bufs[2][64:64 + 16].view(torch.int32).view(1, 4))
        det.detect_into(img, out)
        torch.cuda.synchronize()
        for b, n in zip(bufs, sizes):
            b = b.cpu().numpy()
            assert np.all(b[:64] == 0xA5) and np.all(b[64 + n:] == 0xA5)
        want = qd.detect_batch(img.cpu().numpy(), max_components=maxc, max_quads=maxq)
        same_bytes((out[0].cpu().numpy(), quad_detect.records_numpy(out[1]), out[2].cpu().numpy()), want, "guarded %d %d" % (maxc, maxq))


def test_batch_pitch_stride_and_views(torch_cuda):
    """B = 3 with three different frames: plain, as three B = 1 calls, and as a non-contiguous view (rows 13 bytes longer, a padded
    frame stride) into a buffer with a DARK border, which must not leak into any component"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import quad_detect
    seq = ts.sequence("small")
    frames = np.stack([seq.frame(k) for k in range(3)])
    det = quad_detect.QuadDetector(seq.width, seq.height, max_batch=3)
    plain = device_detect(torch, frames, detector=det)
    same_bytes(plain, qd.detect_batch(frames), "B = 3")
    for k in range(3):
        one = device_detect(torch, frames[k:k + 1], detector=det)
        same_bytes(one, tuple(a[k:k + 1] for a in plain), "frame %d alone" % k)
    buf = torch.zeros((3, seq.height + 9, seq.width + 13), dtype=torch.uint8, device="cuda")
    view = buf[:, 4:4 + seq.height, 5:5 + seq.width]
    view.copy_(torch.from_numpy(frames).cuda())
    assert view.stride(1) == seq.width + 13 and view.stride(0) == (seq.height + 9) * (seq.width + 13) and not view.is_contiguous()
    same_bytes(device_detect(torch, view, detector=det), plain, "view")
    lab = det.labels(view)
    torch.cuda.synchronize()
    assert lab.cpu().numpy()[2].tobytes() == qd.labels(frames[2]).tobytes()


def test_handle_reuse_across_frame_sizes(torch_cuda):
    """1280 x 720, then 64 x 48, then 1280 x 720 on one handle equals fresh handles (nothing stale is read), run after run"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import quad_detect
    big, small = ts.sequence("dense").frame(0)[None], S.single_quad(1)[0][None]
    det = quad_detect.QuadDetector(1280, 720)
    fresh_big, fresh_small = device_detect(torch, big), device_detect(torch, small)
    a, b, c = device_detect(torch, big, detector=det), device_detect(torch, small, detector=det), device_detect(torch, big, detector=det)
    same_bytes(a, fresh_big, "first large"); same_bytes(b, fresh_small, "small after large"); same_bytes(c, fresh_big, "large after small")
    same_bytes(b, qd.detect_batch(small), "small after large against numpy")
    assert b[2][0, 2] == 1


# ---- options

def test_options_at_their_edges(torch_cuda):
    torch = torch_cuda
    img = ts.sequence("small").frame(0)[None]
    base = device_detect(torch, img)
    rec = base[1][0, :base[2][0, 2]]
    area = int(np.sort(rec["area"])[len(rec) // 2])
    cases = [dict(min_contrast=1), dict(min_contrast=255), dict(min_area=area), dict(min_area=area + 1), dict(min_area=area, max_area=area),
             dict(min_fill_pct=0), dict(min_fill_pct=100), dict(min_area=1, min_fill_pct=0, min_contrast=20)]
    seen = {}
    for kw in cases:
        got = device_detect(torch, img, **kw)
        same_bytes(got, qd.detect_batch(img, **kw), str(kw))
        seen[str(kw)] = got[2][0].tolist()
    print(seen)
    n_at, n_above = seen[str(cases[2])][1], seen[str(cases[3])][1]
    assert n_at - n_above == int((qd.component_sums(qd.labels(img[0]))[1] == area).sum()) >= 1
    # a frame that does span 0..255: min_contrast 255 still labels it
    frame = S.pattern_frames(64, 48)[0][S.PATTERNS.index(S.diagonal_blobs)][None]
    got = device_detect(torch, frame, min_contrast=255, min_area=1)
    same_bytes(got, qd.detect_batch(frame, min_contrast=255, min_area=1), "0 / 255 frame at 255")
    assert got[2][0, 0] == 2


def test_argument_errors_by_value(torch_cuda):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import quad_detect, quadfindlib as Q
    det = quad_detect.QuadDetector(64, 48, max_batch=2)
    ok = torch.zeros((1, 48, 64), dtype=torch.uint8, device="cuda")
    for frames in (torch.zeros((1, 7, 64), dtype=torch.uint8, device="cuda"), torch.zeros((1, 48, 7), dtype=torch.uint8, device="cuda"),
                   torch.zeros((3, 48, 64), dtype=torch.uint8, device="cuda"), torch.zeros((1, 49, 64), dtype=torch.uint8, device="cuda")):
        with pytest.raises(Q.QuadFindError, match="AGT_QUADFIND_ERR_ARG"):
            det.detect(frames)
        with pytest.raises(Q.QuadFindError, match="AGT_QUADFIND_ERR_ARG"):
            det.labels(frames)
    for kw in (dict(min_contrast=0), dict(min_contrast=256), dict(min_area=0), dict(min_area=10, max_area=9), dict(min_fill_pct=-1), dict(min_fill_pct=101)):
        with pytest.raises(Q.QuadFindError, match="AGT_QUADFIND_ERR_ARG"):
            det.detect(ok, **kw)
    with pytest.raises(Q.QuadFindError, match="AGT_QUADFIND_ERR_ARG"):
        det.labels(ok, min_contrast=0)
    # the library itself: sizes, batch, pitch, stride and NULL outputs, on a live handle
    fd = det._finder(0)
    good = dict(frames=ok.data_ptr(), pitch=64, stride=64 * 48, w=64, h=48, B=1, quads=64, records=64, counts=64)

    def call(**kw):
        a = dict(good, **kw)
        return fd.L.agt_quadfind_detect(fd.h, None, a["frames"], a["pitch"], a["stride"], a["w"], a["h"], a["B"], None, a["quads"], a["records"], a["counts"])
    for kw in (dict(w=7), dict(h=7), dict(w=65), dict(h=49), dict(B=0), dict(B=3), dict(pitch=63), dict(B=2, stride=64 * 47 + 63), dict(frames=None),
               dict(quads=None), dict(records=None), dict(counts=None)):
        assert call(**kw) == Q.ERR_ARG, kw
    assert fd.L.agt_quadfind_labels(fd.h, None, ok.data_ptr(), 64, 64 * 48, 64, 48, 1, 40, None) == Q.ERR_ARG
    # and the handle still works
    assert device_detect(torch, np.array(S.single_quad(0)[0])[None], detector=det)[2][0, 2] == 1


# ---- the chain and the other doors

@pytest.fixture(scope="module")
def family():
    from accurate_aprilgroup_tracking_amd import tag_decode
    return tag_decode.TagFamily(ts.family_codes(), "synthetic36")


@pytest.mark.parametrize("name,k", [("small", 0), ("small", 1), ("dense", 0)])
def test_chain_finds_every_front_tag_with_its_id(torch_cuda, family, name, k):
    """find -> refine -> decode on the device: every tag seen at under 60 degrees comes back with its id, its corners within
    max(0.35 px, 1.1 x what the numpy chain of tests/quad_detect_scenes.py reaches on the frame); no candidate carries an id the
    scene does not hold"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import tag_detect
    seq = ts.sequence(name)
    chain = S.numpy_chain(name, k)
    tags = tag_detect.detect_tags(torch.from_numpy(seq.frame(k)[None]).cuda(), family)
    torch.cuda.synchronize()
    ok, ids, rot = tags.ok.cpu().numpy()[0], tags.ids.cpu().numpy()[0], tags.rotations.cpu().numpy()[0]
    quads, margins = tags.quads.cpu().numpy()[0].astype(np.float64), tags.margins.cpu().numpy()[0]
    truth = ts.quads(seq, k).astype(np.float64)
    T = len(truth)
    assert ok.sum() > 0 and np.all(ids[ok == 1] >= 0) and np.all(ids[ok == 1] < T), "an id that is not in the scene"
    assert not ok[int(tags.found.counts.cpu().numpy()[0, 2]):].any()
    worst = 0.0
    for t in chain["front"]:
        slots = np.nonzero((ok == 1) & (ids == t))[0]
        assert len(slots) == 1, "tag %d: %d candidates" % (t, len(slots))
        q = np.roll(quads[slots[0]], rot[slots[0]], axis=0)
        worst = max(worst, np.linalg.norm(q - truth[t], axis=1).max())
    bound = max(S.REFINED_PX, 1.1 * chain["refined"].max())
    print("%s %d: %d front tags, %d decoded, device chain worst corner %.3f px, numpy chain %.3f px, bound %.3f px, smallest margin %.1f" %
          (name, k, len(chain["front"]), int(ok.sum()), worst, chain["refined"].max(), bound, margins[ok == 1].min()))
    assert worst <= bound


def test_tracker_acquires_from_nothing(torch_cuda, family):
    """a cold StreamTracker: detect_tags -> step_detected is accepted, mask bytes are 1 exactly for the tags that were found and 0 for
    those facing away, and the next step() on frame 1 is accepted"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H, tag_decode
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    seq = ts.sequence("small")
    T = len(seq.obj) // 4
    frame0, frame1 = (torch.from_numpy(seq.frame(k)[None]).cuda().contiguous() for k in (0, 1))
    trk = StreamTracker(seq.width, seq.height, seq.obj, seq.K, seq.dist, n_streams=1)
    trk.reset()
    corners, cmask, records = trk.detect_tags(frame0, family)
    assert corners.shape == (1, trk.n, 2) and corners.dtype == torch.float32 and corners.is_contiguous() and cmask.shape == (1, trk.n) and cmask.dtype == torch.uint8
    s0, s1 = trk.new_state_buffer(), trk.new_state_buffer()
    trk.step_detected(frame0, corners, cmask, s0)
    trk.step(frame1, s1)
    trk.join()
    torch.cuda.synchronize()
    m = cmask.cpu().numpy()[0].reshape(T, 4)
    rec = tag_decode.records_numpy(records)[0]
    found = sorted(set(int(i) for i in rec["id"][rec["status"] == 0]))
    assert np.all((m == 0) | (m == 1)) and np.all(m.min(axis=1) == m.max(axis=1))
    assert sorted(np.nonzero(m[:, 0])[0].tolist()) == found, "mask bytes are 1 exactly for the tags that decoded"
    cos = ts.view_cosines(seq, 0)
    assert set(ts.front_tags(seq, 0)) <= set(found) and not m[cos <= 0.0].any()
    c = corners.cpu().numpy()[0].reshape(T, 4, 2)
    truth = ts.quads(seq, 0)
    front = ts.front_tags(seq, 0)
    err = np.linalg.norm(c[front] - truth[front], axis=2).max()
    assert not c[m[:, 0] == 0].any()
    s0, s1 = s0.cpu().numpy()[0], s1.cpu().numpy()[0]
    e0 = float(np.linalg.norm(s0[H.ST_TVEC:H.ST_TVEC + 3] - seq.tvecs[0])); e1 = float(np.linalg.norm(s1[H.ST_TVEC:H.ST_TVEC + 3] - seq.tvecs[1]))
    print("%d tags found of %d (front: %d), worst front-tag corner %.3f px in model order; translation error %.5f m on the detected frame, %.5f m after step()" %
          (len(found), T, len(ts.front_tags(seq, 0)), err, e0, e1))
    assert err <= max(S.REFINED_PX, 1.1 * S.numpy_chain("small", 0)["refined"].max())
    assert s0[H.ST_OK] == 1.0 and s1[H.ST_OK] == 1.0


def test_duplicate_ids_larger_margin_wins(torch_cuda):
    """corner_table on made-up candidates: two with one id (the larger margin wins), a tie (the lower slot wins), an id outside the
    model, a candidate that is not ok; corners rolled by the rotation"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import tag_detect
    Q = 7
    quads = torch.arange(Q * 8, dtype=torch.float32, device="cuda").view(1, Q, 4, 2) + 1.0
    ids = torch.tensor([[2, 2, 0, 0, 9, 1, -1]], dtype=torch.int32, device="cuda")
    rot = torch.tensor([[0, 1, 2, 3, 0, 0, -1]], dtype=torch.int32, device="cuda")
    margins = torch.tensor([[50.0, 60.0, 70.0, 70.0, 99.0, 80.0, 0.0]], dtype=torch.float64, device="cuda")
    ok = torch.tensor([[1, 1, 1, 1, 1, 0, 0]], dtype=torch.uint8, device="cuda")
    tags = tag_detect.Tags(quads, ids, rot, margins, ok, None, None, None)
    lut = torch.tensor([0, 1, 2, -1, -1, -1, -1, -1, -1, -1], dtype=torch.int64, device="cuda")
    corners, mask = tag_detect.corner_table(tags, lut, 3)
    torch.cuda.synchronize()
    q, c = quads.cpu().numpy()[0], corners.cpu().numpy()[0].reshape(3, 4, 2)
    assert mask.cpu().numpy()[0].reshape(3, 4).tolist() == [[1] * 4, [0] * 4, [1] * 4]
    assert np.array_equal(c[0], np.roll(q[2], 2, axis=0)) and np.array_equal(c[2], np.roll(q[1], 1, axis=0)) and not c[1].any()


def test_pose_detector_with_the_device_tag_detector(torch_cuda, family, tmp_path):
    """PoseDetector(..., detector=DeviceTagDetector(family)) runs the detector-fed path with no outside module and accepts frame 0"""
    import json
    import logging
    from accurate_aprilgroup_tracking_amd import tag_detect
    from accurate_aprilgroup_tracking_amd.pose_detector import PoseDetector
    seq = ts.sequence("small")
    (tmp_path / "april_group.json").write_text(json.dumps(seq.group))

    class Det(PoseDetector):
        DIRPATH = str(tmp_path)
    log = logging.getLogger("test_gpu_quad_detect"); log.setLevel(logging.CRITICAL)
    detector = tag_detect.DeviceTagDetector(family)
    found = detector(seq.frame(0))
    truth = ts.quads(seq, 0).astype(np.float64)
    assert set(ts.front_tags(seq, 0)) <= {d.tag_id for d in found} <= set(range(len(truth)))
    for d in found:
        assert np.asarray(d.corners).shape == (4, 2) and d.decision_margin > 0
        if d.tag_id in ts.front_tags(seq, 0):
            assert np.linalg.norm(np.asarray(d.corners) - truth[d.tag_id], axis=1).max() <= 0.5, "corners in the tag's own order"
    det = Det(log, seq.K, None, True, detector=detector, backend="stream")
    det._detect_and_get_pose(seq.frame(0))
    assert det.last_pose[0] is not None, "frame 0 accepted"
    e = float(np.linalg.norm(np.asarray(det.last_pose[1], np.float64).ravel() - seq.tvecs[0]))
    print("PoseDetector + DeviceTagDetector on small 0: %d detections, translation error %.5f m" % (len(found), e))
    assert e < 0.05, "a sanity bound only: the scene is 0.6 m deep"


def test_cv_detect_quads_equals_quad_detector(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    img = ts.sequence("small").frame(0)
    quads, rec = cv_hip.detectQuads(img)
    got = device_detect(torch_cuda, img[None])
    n = int(got[2][0, 2])
    assert quads.dtype == np.float32 and quads.shape == (n, 4, 2) and quads.tobytes() == got[0][0, :n].tobytes() and rec.tobytes() == got[1][0, :n].tobytes()
    quads, rec = cv_hip.detectQuads(img, max_quads=5, min_contrast=60)
    got = device_detect(torch_cuda, img[None], max_quads=5, min_contrast=60)
    assert quads.tobytes() == got[0][0].tobytes() and rec.tobytes() == got[1][0].tobytes() and len(rec) == 5
    quads, rec = cv_hip.detectQuads(np.full((48, 64), 200, np.uint8))
    assert quads.shape == (0, 4, 2) and rec.shape == (0,) and rec.dtype == qd.RECORD_DTYPE
    for bad in (img.astype(np.float32), img[None]):
        with pytest.raises(cv_hip.error):
            cv_hip.detectQuads(bad)
    with pytest.raises(cv_hip.error, match="AGT_QUADFIND_ERR_ARG"):
        cv_hip.detectQuads(img, min_contrast=0)
    with pytest.raises(cv_hip.error, match="AGT_QUADFIND_ERR_ARG"):
        cv_hip.detectQuads(img[:7])
    with pytest.raises(cv_hip.error, match="unknown"):
        cv_hip.detectQuads(img, minContrast=3)
