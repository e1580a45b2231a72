"""-m gpu: the tag decode kernel (include/agt_tagcode.h) against the numpy statement of its rule (tests/tag_decode_numpy.py) on the
rendered scenes of tests/tag_decode_scenes.py, at the shapes where the lane mapping can go wrong, on quads that must be refused by
value, and through its three public doors (tag_decode.decode_quads, cv_hip.decodeTags, StreamTracker.decode_tags)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import tag_decode_numpy as tn      # noqa: E402
import tag_decode_scenes as ts     # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9               # the project's FP64 bound: values of at most 255, fixed and well conditioned normal equations
BIT_FLOOR = 1e-6         # a bit is compared only where the numpy statement's |I - thr| exceeds this
READ = (tn.OK, tn.NO_MATCH, tn.LOW_MARGIN)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    torch.cuda.set_device(0)
    return torch


@pytest.fixture(scope="module")
def family():
    from accurate_aprilgroup_tracking_amd import tag_decode
    return tag_decode.TagFamily(ts.family_codes(), "synthetic36")


def device_decode(torch, frames, quads, family, mask=None, expected=None, **kw):
    """host arrays (or a cuda frame tensor) in -> (records [B, Q] structured, ok [B, Q], corner_mask [B, 4Q], H [B, Q, 3, 3])"""
    from accurate_aprilgroup_tracking_amd import tag_decode
    f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = tag_decode.decode_quads(f, torch.from_numpy(np.ascontiguousarray(quads, np.float32)).cuda(), family,
                                  mask=None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda(),
                                  expected=None if expected is None else torch.from_numpy(np.ascontiguousarray(expected, np.int32)).cuda(), **kw)
    torch.cuda.synchronize()
    return tag_decode.records_numpy(out.records), out.ok.cpu().numpy(), out.corner_mask.cpu().numpy(), out.homography.cpu().numpy()


def payload_mask(d):
    """word mask of the payload cells whose |I - thr| exceeds BIT_FLOOR"""
    return tn.word_of([[abs(d[(r, c)]) > BIT_FLOOR for c in range(1, 7)] for r in range(1, 7)])


def compare(got, want, max_excluded=0):
    """device results against the numpy statement's, quad by quad -> the number of quads with a payload bit left out"""
    rec, ok, cmask, H = got
    B, Q = rec.shape
    assert (len(want), len(want[0])) == (B, Q) and ok.shape == (B, Q) and cmask.shape == (B, 4 * Q) and H.shape == (B, Q, 3, 3)
    assert np.array_equal(cmask, np.repeat(ok, 4, axis=1))
    excluded = 0
    worst = dict(margin=0.0, contrast=0.0, H=0.0)
    for b in range(B):
        for q in range(Q):
            g, w, where = rec[b, q], want[b][q], "entry %d quad %d" % (b, q)
            full = w["d"] is None or payload_mask(w["d"]) == (1 << 36) - 1
            if not full:
                # a bit too close to its threshold: what does not hang on it is still compared
                excluded += 1
                m = payload_mask(w["d"])
                assert g["status"] in READ and (int(g["word"]) & m) == (w["word"] & m), where
                continue
            assert int(g["status"]) == w["status"], "%s: status %d, numpy %d" % (where, g["status"], w["status"])
            assert (int(g["word"]), int(g["id"]), int(g["hamming"]), int(g["rot"])) == (w["word"], w["id"], w["hamming"], w["rot"]), where
            assert int(ok[b, q]) == w["ok"], where
            worst["margin"] = max(worst["margin"], abs(g["margin"] - w["margin"]))
            worst["contrast"] = max(worst["contrast"], abs(g["contrast"] - w["contrast"]))
            if np.any(w["H"]):
                assert H[b, q, 2, 2] != 0.0, where
                worst["H"] = max(worst["H"], np.abs(H[b, q] / H[b, q, 2, 2] - w["H"] / w["H"][2, 2]).max())
            else:
                assert not np.any(H[b, q]), where
    print("largest differences: margin %.3g contrast %.3g H %.3g; %d of %d quads with a bit left out" % (worst["margin"], worst["contrast"], worst["H"], excluded, B * Q))
    assert worst["margin"] <= TOL and worst["contrast"] <= TOL and worst["H"] <= TOL
    assert excluded <= max_excluded
    return excluded


TAG_CASES = {"small": (0, 1), "dense": (0,)}


@pytest.mark.parametrize("noise", [0.0, 0.5])
@pytest.mark.parametrize("name", sorted(TAG_CASES))
def test_parity_on_tag_scenes(torch_cuda, family, name, noise):
    """every quad of the scene (tags that face away included): all fields, no quad left out; the front-facing tags decode"""
    seq, ks = ts.sequence(name), TAG_CASES[name]
    frames = np.stack([seq.frame(k) for k in ks])
    quads = np.stack([ts.quads(seq, k, noise) for k in ks])
    expected = np.arange(quads.shape[1], dtype=np.int32)
    want = tn.decode(frames, quads, ts.family_codes(), expected=expected, min_margin=30.0)
    got = device_decode(torch_cuda, frames, quads, family, expected=expected, min_margin=30.0)
    compare(got, want, 0)
    for b, k in enumerate(ks):
        front = ts.front_tags(seq, k)
        assert np.all(got[1][b, front] == 1) and np.array_equal(got[0]["id"][b, front], front) and np.all(got[0]["rot"][b, front] == 0)


@pytest.mark.parametrize("name", ["small", "dense"])
def test_parity_on_background_quads(torch_cuda, family, name):
    seq = ts.sequence(name)
    frames, quads = ts.bare_frame(seq)[None], ts.background_quads(seq, 64)[None]
    want = tn.decode(frames, quads, ts.family_codes())
    got = device_decode(torch_cuda, frames, quads, family)
    compare(got, want, max_excluded=1)             # 2 % of 64
    assert not got[1].any()


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Q", [1, 3, 4, 5])
def test_quad_counts_around_the_workgroup(torch_cuda, family, B, Q):
    """four waves per workgroup: Q * B below, at and above it, the last workgroup part filled"""
    seq = ts.sequence("small")
    frames = np.stack([seq.frame(k) for k in range(B)])
    quads = np.stack([ts.quads(seq, k)[2:2 + Q] for k in range(B)])
    expected = np.arange(2, 2 + Q, dtype=np.int32)
    compare(device_decode(torch_cuda, frames, quads, family, expected=expected), tn.decode(frames, quads, ts.family_codes(), expected=expected))


@pytest.mark.parametrize("which", ["first", "last", "all"])
def test_mask_bytes(torch_cuda, family, which):
    seq = ts.sequence("small")
    frames = np.stack([seq.frame(k) for k in range(2)])
    quads = np.stack([ts.quads(seq, k)[:5] for k in range(2)])
    mask = np.ones((2, 5), np.uint8)
    if which == "first":
        mask[:, 0] = 0
    elif which == "last":
        mask[:, -1] = 0
    else:
        mask[:] = 0
    got = device_decode(torch_cuda, frames, quads, family, mask=mask)
    compare(got, tn.decode(frames, quads, ts.family_codes(), mask=mask))
    assert np.array_equal(got[0]["status"] == tn.MASKED, mask == 0) and np.array_equal(got[1], mask)
    masked = got[0][mask == 0]
    assert np.all(masked["id"] == -1) and np.all(masked["hamming"] == -1) and np.all(masked["rot"] == -1)
    assert not masked["word"].any() and not masked["margin"].any() and not masked["contrast"].any()


@pytest.mark.parametrize("n_codes", [1, 15, 16, 17, 587])
def test_match_in_the_last_slot(torch_cuda, n_codes):
    """4 n candidates either side of the 64 lanes and many trips of the search loop; the tag's code sits last"""
    from accurate_aprilgroup_tracking_amd import synthetic as syn, tag_decode
    seq = ts.sequence("small")
    tag = int(ts.front_tags(seq, 0)[0])
    own = ts.family_codes()[tag]
    others = syn.make_tag_family(587, 9, 5)[:n_codes - 1]
    assert all(bin(cw ^ int(own)).count("1") > 2 for _, _, cw in tn.candidates(others))
    codes = np.append(others, own).astype(np.uint64)
    frames, quads = seq.frame(0)[None], np.stack([np.roll(ts.quads(seq, 0)[tag], -k, axis=0) for k in range(4)])[None]
    got = device_decode(torch_cuda, frames, quads, tag_decode.TagFamily(codes))
    compare(got, tn.decode(frames, quads, codes))
    assert np.all(got[0]["id"] == n_codes - 1) and np.array_equal(got[0]["rot"][0], np.arange(4)) and np.all(got[0]["hamming"] == 0)


def test_duplicated_code_returns_the_lower_index(torch_cuda):
    from accurate_aprilgroup_tracking_amd import tag_decode
    seq, codes = ts.sequence("small"), ts.family_codes()
    tag = int(ts.front_tags(seq, 0)[0])
    dup = np.concatenate([codes[40:60], codes[tag:tag + 1], codes[20:40], codes[tag:tag + 1]])
    got = device_decode(torch_cuda, seq.frame(0)[None], ts.quads(seq, 0)[tag][None, None], tag_decode.TagFamily(dup))
    assert (got[0]["id"][0, 0], got[0]["rot"][0, 0], got[0]["hamming"][0, 0]) == (20, 0, 0)


@pytest.mark.parametrize("fill", [0, 255])
def test_pitch_and_views_inside_a_larger_buffer(torch_cuda, family, fill):
    """rows 13 bytes longer than the frame, frames inside a buffer with a border of `fill`: nothing outside the frame is read"""
    torch = torch_cuda
    seq = ts.sequence("small")
    frames = np.stack([seq.frame(k) for k in range(2)])
    quads = np.stack([np.concatenate([ts.quads(seq, k), ts.background_quads(seq, 20, k)]) for k in range(2)])
    # quads whose rings end on the last readable column and row
    m = 1.125 * 16
    for slot, (x, y) in ((-1, (m, m)), (-2, (seq.width - 2 - m, seq.height - 2 - m))):
        quads[:, slot] = np.array([[x - 16, y - 16], [x - 16, y + 16], [x + 16, y + 16], [x + 16, y - 16]], np.float32)
    plain = device_decode(torch, frames, quads, family)
    buf = torch.full((2, seq.height + 9, seq.width + 13), fill, dtype=torch.uint8, device="cuda")
    view = buf[:, 4:4 + seq.height, :seq.width]
    view.copy_(torch.from_numpy(frames).cuda())
    assert view.stride(1) == seq.width + 13 and view.stride(0) == (seq.height + 9) * (seq.width + 13)
    got = device_decode(torch, view, quads, family)
    assert plain[0].tobytes() == got[0].tobytes() and np.array_equal(plain[3].view(np.uint64), got[3].view(np.uint64))
    assert np.array_equal(plain[1], got[1]) and np.array_equal(plain[2], got[2])
    assert np.all(plain[0]["status"][:, -2:] != tn.OUTSIDE) and np.all(plain[0]["status"][:, -2:] != tn.DEGENERATE)
    compare(plain, tn.decode(frames, quads, ts.family_codes()), max_excluded=0)


def test_bad_quads_are_refused_by_value(torch_cuda, family):
    seq = ts.sequence("small")
    sq = np.array([[100.0, 100.0], [100.0, 140.0], [140.0, 140.0], [140.0, 100.0]], np.float32)
    quads = []
    for bad in (np.nan, np.inf, -np.inf, 1e30, -1e30):
        for slot in range(8):
            q = sq.copy(); q.reshape(-1)[slot] = bad
            quads.append(q)
    quads.append(np.full((4, 2), np.nan, np.float32))
    quads.append(np.full((4, 2), 1e30, np.float32))
    n_value = len(quads)
    quads += [np.repeat(sq[:1], 4, axis=0), np.array([[0, 0], [10, 10], [20, 20], [30, 30]], np.float32), sq[[0, 2, 1, 3]], sq[[0, 1, 1, 3]],
              sq[[0, 0, 2, 3]], np.zeros((4, 2), np.float32)]
    quads = np.stack(quads)[None]
    frames = seq.frame(0)[None]
    got = device_decode(torch_cuda, frames, quads, family)
    assert np.all(got[0]["status"] == tn.DEGENERATE), got[0]["status"]
    assert not got[1].any() and not got[3].any() and np.all(got[0]["id"] == -1)
    compare(got, tn.decode(frames, quads, ts.family_codes()))
    assert n_value == 42


def edge_frame():
    """200 x 160, four axis-aligned tags of 6 px cells whose outermost ring samples fall on the first / last readable column or row"""
    w, h, cell = 200, 160, 6
    frame = np.full((h, w), 128, np.uint8)
    bits = ts.syn.family_bits(ts.family_codes(), np.arange(4))
    quads = []
    for t, (cx, cy) in enumerate(((27, 80), (w - 29, 80), (100, 27), (100, h - 29))):
        pat = np.full((10, 10), 225, np.uint8)
        pat[1:9, 1:9] = 30
        pat[2:8, 2:8] = np.where(bits[t] > 0, 225, 30)
        for py in range(max(cy - 30, 0), min(cy + 30, h)):
            for px in range(max(cx - 30, 0), min(cx + 30, w)):
                frame[py, px] = pat[(py - (cy - 30)) // cell, (px - (cx - 30)) // cell]
        quads.append([[cx - 24, cy - 24], [cx - 24, cy + 24], [cx + 24, cy + 24], [cx + 24, cy - 24]])
    return frame, np.array(quads, np.float32)


def test_ring_one_pixel_outside_is_refused(torch_cuda, family):
    frame, inside = edge_frame()
    shift = np.array([[-1, 0], [1, 0], [0, -1], [0, 1]], np.float32)
    quads = np.concatenate([inside, inside + shift[:, None, :]])[None]
    got = device_decode(torch_cuda, frame[None], quads, family)
    print("status", got[0]["status"][0], "margin", got[0]["margin"][0])
    assert np.all(got[0]["status"][0, :4] == tn.OK) and np.array_equal(got[0]["id"][0, :4], np.arange(4)) and np.all(got[0]["rot"][0, :4] == 0)
    assert np.all(got[0]["status"][0, 4:] == tn.OUTSIDE) and np.all(got[0]["id"][0, 4:] == -1) and not got[0]["word"][0, 4:].any()
    compare(got, tn.decode(frame[None], quads, ts.family_codes()))


def test_two_runs_are_bitwise_equal(torch_cuda, family):
    seq = ts.sequence("dense")
    frames = seq.frame(0)[None]
    quads = np.concatenate([ts.quads(seq, 0, 0.5), ts.background_quads(seq, 64)])[None]
    a, b = device_decode(torch_cuda, frames, quads, family), device_decode(torch_cuda, frames, quads, family)
    assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[3].view(np.uint64), b[3].view(np.uint64))
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])


def test_cv_decode_tags_returns_the_numpy_detections(torch_cuda, family):
    from accurate_aprilgroup_tracking_amd import cv_hip
    seq = ts.sequence("small")
    q = ts.quads(seq, 0, 0.5)
    quads = np.concatenate([q, ts.background_quads(seq, 8), np.stack([np.roll(q[i], -(i % 4), axis=0) for i in range(4)])])
    dets = cv_hip.decodeTags(seq.frame(0), quads, family, maxHamming=2, minMargin=30.0)
    want = [(quad, r) for quad, r in zip(quads, tn.decode(seq.frame(0)[None], quads[None], ts.family_codes(), min_margin=30.0)[0]) if r["status"] == tn.OK]
    assert len(dets) == len(want) >= len(ts.front_tags(seq, 0)) + 4
    for d, (quad, r) in zip(dets, want):
        assert (d.tag_id, d.hamming, d.tag_family) == (r["id"], r["hamming"], b"synthetic36")
        assert abs(d.decision_margin - r["margin"]) <= TOL
        assert np.array_equal(d.corners, np.roll(quad, r["rot"], axis=0).astype(np.float64))
        proj = np.c_[tn.SQUARE, np.ones(4)] @ d.homography.T
        assert np.abs(proj[:, :2] / proj[:, 2:] - d.corners).max() < 1e-8
        Hn = r["H"] / r["H"][2, 2]
        assert np.abs(d.center - Hn[:2, 2]).max() <= TOL
    assert cv_hip.decodeTags(seq.frame(0), np.zeros((0, 4, 2)), family) == []
    with pytest.raises(cv_hip.error):
        cv_hip.decodeTags(seq.frame(0).astype(np.float32), quads, family)


def test_tracker_decode_tags(torch_cuda, family):
    """the tracker's own corners after three LK steps decode to their tags; a tag whose corners were overwritten with a neighbour's
    loses its four mask bytes, and the pose solve with that mask is accepted"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H, tag_decode
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    seq = ts.sequence("small")
    T = len(seq.obj) // 4
    trk = StreamTracker(seq.width, seq.height, seq.obj, seq.K, seq.dist, n_streams=1)
    up = lambda k: torch.from_numpy(seq.frame(k)[None]).cuda().contiguous()
    trk.reset(up(0), torch.from_numpy(seq.corners(0)[None]).cuda().contiguous())
    for k in (1, 2, 3):
        trk.step(up(k))
    last = up(3)
    records, cmask = trk.decode_tags(last, family, tag_ids=np.arange(T))
    torch.cuda.synchronize()
    rec, cm = tag_decode.records_numpy(records)[0], cmask.cpu().numpy()[0]
    front = ts.front_tags(seq, 3)
    print("after three steps: status %s margin %s" % (rec["status"], np.round(rec["margin"], 1)))
    assert cmask.shape == (1, trk.n) and len(front) >= 8
    assert np.array_equal(rec["id"][front], front) and np.all(rec["rot"][front] == 0) and np.all(rec["status"][front] == tn.OK)
    assert np.all(cm.reshape(T, 4)[front] == 1)
    # tag a takes the corners of its neighbour b
    a, b = int(front[0]), int(front[1])
    c = np.zeros((1, trk.n, 2), np.float32)
    H.check(trk.ctx.L.agt_download(trk.ctx.h, c.ctypes.data_as(C.c_void_p), C.c_void_p(trk.corners()[0]), c.nbytes), "agt_download")
    c[0, 4 * a:4 * a + 4] = c[0, 4 * b:4 * b + 4]
    corners = torch.from_numpy(c).cuda().contiguous()
    ones = torch.ones((1, trk.n), dtype=torch.uint8, device="cuda")
    trk.step_detected(last, corners, ones)
    records, cmask = trk.decode_tags(last, family, tag_ids=np.arange(T))
    so = trk.new_state_buffer()
    trk.estimate_pose(corners, cmask, so)
    torch.cuda.synchronize()
    rec, cm = tag_decode.records_numpy(records)[0], cmask.cpu().numpy()[0].reshape(T, 4)
    assert rec["status"][a] == tn.OK and rec["id"][a] == b                  # it reads the neighbour's payload
    want = np.zeros(T, np.uint8); want[front] = 1; want[a] = 0
    assert np.array_equal(cm, np.repeat(want[:, None], 4, axis=1))
    state = so.cpu().numpy()[0]
    print("pose with the decode mask: ok %d err %.3f px" % (state[H.ST_OK], state[H.ST_ERR]))
    assert state[H.ST_OK] == 1.0
