"""-m gpu: the quad refinement kernel (include/agt_quadfit.h) against the numpy statement of its rule (tests/quad_refine_numpy.py) on
the rendered scenes of tests/tag_decode_scenes.py, at the shapes where the lane mapping can go wrong, on quads that must be refused by
value, and through its three public doors (quad_refine.refine_quads, cv_hip.refineQuads, StreamTracker.refine_tags)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quad_refine_numpy as qn     # noqa: E402
import tag_decode_scenes as ts     # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 1e-9               # the project's FP64 bound: corners of at most a few thousand pixels, sums of at most 17 squares of 255
NEAR = 1e-6              # a quad is compared by value only where the numpy statement shows every decision further than this from flipping
SEED = 3


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    if not torch.cuda.is_available():
        pytest.fail("needs a GPU")
    torch.cuda.set_device(0)
    return torch


def device_refine(torch, frames, quads, mask=None, **kw):
    """host arrays (or a cuda frame tensor) in -> (records [B, Q] structured, quads f32, quads64, ok [B, Q], corner_mask [B, 4Q])"""
    from accurate_aprilgroup_tracking_amd import quad_refine
    f = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    out = quad_refine.refine_quads(f, torch.from_numpy(np.ascontiguousarray(quads, np.float32)).cuda(),
                                   mask=None if mask is None else torch.from_numpy(np.ascontiguousarray(mask, np.uint8)).cuda(), **kw)
    torch.cuda.synchronize()
    assert out.quads.is_contiguous() and out.quads.dtype == torch.float32
    return quad_refine.records_numpy(out.records), out.quads.cpu().numpy(), out.quads64.cpu().numpy(), out.ok.cpu().numpy(), out.corner_mask.cpu().numpy()


def near_a_decision(r, min_strength):
    n = r["notes"]
    return r["status"] in (qn.OK, qn.WEAK, qn.DIVERGED) and (abs(r["strength"] - min_strength) <= NEAR or n["frame_limit"] <= NEAR or n["Mc"] <= NEAR)


def compare(got, want, quads_in, min_strength=40.0, max_excluded=0):
    """device results against the numpy statement's, quad by quad -> (quads left out of the value comparison, largest differences)"""
    rec, q32, q64, ok, cmask = got
    B, Q = rec.shape
    quads_in = np.asarray(quads_in, np.float32)
    assert (len(want), len(want[0])) == (B, Q) and q32.shape == q64.shape == (B, Q, 4, 2) and ok.shape == (B, Q) and cmask.shape == (B, 4 * Q)
    assert np.array_equal(cmask, np.repeat(ok, 4, axis=1)) and np.array_equal(ok, (rec["status"] == qn.OK).astype(np.uint8))
    excluded, worst = 0, dict(quads64=0.0, strength=0.0, shift=0.0, resid=0.0)
    for b in range(B):
        for q in range(Q):
            r, g = want[b][q], rec[b, q]
            where = "quad (%d, %d): device %s, numpy %s" % (b, q, g, {k: r[k] for k in ("status", "passes", "strength", "shift", "resid")})
            if g["status"] != qn.OK:
                assert q32[b, q].tobytes() == quads_in[b, q].tobytes(), where
                assert np.array_equal(q64[b, q], quads_in[b, q].astype(np.float64), equal_nan=True), where
            else:
                # the f32 corners are the f64 ones rounded once
                assert np.all(np.abs(q32[b, q].astype(np.float64) - q64[b, q]) <= np.spacing(np.abs(q64[b, q]).astype(np.float32))), where
            if near_a_decision(r, min_strength):
                excluded += 1
                if g["status"] == qn.WEAK:
                    continue
            assert g["status"] == r["status"] and g["passes"] == r["passes"], where
            for k in ("strength", "shift", "resid"):
                worst[k] = max(worst[k], abs(g[k] - r[k]))
            if r["status"] == qn.OK:
                worst["quads64"] = max(worst["quads64"], np.abs(q64[b, q] - r["quad64"]).max())
    print("left out %d of %d; largest |device - numpy|: %s" % (excluded, B * Q, {k: "%.2e" % v for k, v in worst.items()}))
    assert excluded <= max_excluded
    assert all(v <= TOL for v in worst.values()), worst
    return excluded, worst


TAG_CASES = [("small", 0, 0.0), ("small", 0, 1.0), ("small", 0, 2.0), ("small", 1, 0.0), ("small", 1, 1.0), ("small", 1, 2.0),
             ("dense", 0, 1.0), ("c2", 0, 1.0)]


@pytest.mark.parametrize("name,k,noise", TAG_CASES)
def test_parity_on_tag_scenes(torch_cuda, name, k, noise):
    """every tag of the scene (those facing away included); no quad may be left out.  Measured on the MI355X: none left out (background quads
    included), largest difference 5.7e-14 px (corners), 8.5e-14 (strength), 7.1e-14 (shift), 4.9e-15 (residual) over this file"""
    seq = ts.sequence(name)
    frames, quads = seq.frame(k)[None], ts.quads(seq, k, noise=noise, seed=SEED)[None]
    got = device_refine(torch_cuda, frames, quads)
    front = ts.front_tags(seq, k)
    if noise <= 1.0:
        assert np.all(got[0]["status"][0, front] == qn.OK) and np.all(got[0]["strength"][0, front] >= 80.0)
    compare(got, qn.refine(frames, quads), quads, max_excluded=0)


def test_parity_on_background_quads(torch_cuda):
    seq = ts.sequence("small")
    frames, quads = ts.bare_frame(seq)[None], ts.background_quads(seq, 48)[None]
    got = device_refine(torch_cuda, frames, quads)
    assert np.all(got[0]["status"] == qn.WEAK) and not got[3].any() and got[1].tobytes() == quads.tobytes()
    compare(got, qn.refine(frames, quads), quads, max_excluded=48)


@pytest.mark.parametrize("B,Q", [(1, 1), (1, 5), (1, 7), (3, 5)])
def test_quad_counts_around_the_workgroup(torch_cuda, B, Q):
    """Q = 5 and 7 leave the last workgroup partly empty; B = 3 puts a batch boundary inside a workgroup"""
    seq = ts.sequence("small")
    frames = np.stack([seq.frame(k) for k in range(B)])
    quads = np.stack([ts.quads(seq, k, noise=1.0, seed=SEED)[ts.front_tags(seq, k)[:Q]] for k in range(B)])
    assert quads.shape == (B, Q, 4, 2)
    got = device_refine(torch_cuda, frames, quads)
    assert np.all(got[0]["status"] == qn.OK)
    compare(got, qn.refine(frames, quads), quads)


def test_pitch_stride_and_views_inside_a_larger_buffer(torch_cuda):
    """B = 3, rows 13 bytes longer than the frame, a padded frame stride, a non-contiguous view into a buffer with a bright border:
    the same bits as from plain frames"""
    torch = torch_cuda
    seq = ts.sequence("small")
    frames = np.stack([seq.frame(k) for k in range(3)])
    quads = np.stack([np.concatenate([ts.quads(seq, k, noise=1.0, seed=SEED), ts.background_quads(seq, 3, k)]) for k in range(3)])
    plain = device_refine(torch, frames, quads)
    buf = torch.full((3, seq.height + 9, seq.width + 13), 255, dtype=torch.uint8, device="cuda")
    view = buf[:, 4:4 + seq.height, :seq.width]
    view.copy_(torch.from_numpy(frames).cuda())
    assert view.stride(1) == seq.width + 13 and view.stride(0) == (seq.height + 9) * (seq.width + 13) and not view.is_contiguous()
    got = device_refine(torch, view, quads)
    for a, b in zip(plain, got):
        assert a.tobytes() == b.tobytes()
    compare(plain, qn.refine(frames, quads), quads, max_excluded=9)


def test_mask_bytes(torch_cuda):
    """alternating zeros in one batch entry, another entry all masked: MASKED, corners untouched, the others as without a mask"""
    seq = ts.sequence("small")
    frames = np.stack([seq.frame(0), seq.frame(1)])
    quads = np.stack([ts.quads(seq, k, noise=1.0, seed=SEED) for k in range(2)])
    Q = quads.shape[1]
    mask = np.ones((2, Q), np.uint8)
    mask[0, ::2] = 0
    mask[1, :] = 0
    got, free = device_refine(torch_cuda, frames, quads, mask=mask), device_refine(torch_cuda, frames, quads)
    assert np.all(got[0]["status"][mask == 0] == qn.MASKED) and not got[3][mask == 0].any()
    assert got[0][mask == 1].tobytes() == free[0][mask == 1].tobytes() and got[2][mask == 1].tobytes() == free[2][mask == 1].tobytes()
    compare(got, qn.refine(frames, quads, mask=mask), quads)


def render_quad(w, h, quad, ss=4):
    """a black (30) convex quad on white (225), ss x ss supersampled"""
    q = np.asarray(quad, np.float64)
    sgn = np.sign(sum(q[e][0] * q[(e + 1) % 4][1] - q[(e + 1) % 4][0] * q[e][1] for e in range(4)))
    ys, xs = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cover = np.zeros((h, w))
    for oy in (np.arange(ss) + 0.5) / ss - 0.5:
        for ox in (np.arange(ss) + 0.5) / ss - 0.5:
            inside = np.ones((h, w), bool)
            for e in range(4):
                a, b = q[e], q[(e + 1) % 4]
                inside &= sgn * ((b[0] - a[0]) * (ys + oy - a[1]) - (b[1] - a[1]) * (xs + ox - a[0])) >= 0
            cover += inside
    return np.clip(np.rint(225 - 195 * cover / (ss * ss)), 0, 255).astype(np.uint8)


def test_quads_at_the_frame_borders(torch_cuda):
    """a square turned by 25 degrees at each border of a 200 x 160 frame: 1.5 px inside (nothing dropped), a vertex 10 px outside
    (stations dropped, at least 8 left on every edge: OK) and its centre on the border (WEAK, corners untouched)"""
    w, h = 200, 160
    c, s = np.cos(np.deg2rad(25.0)), np.sin(np.deg2rad(25.0))
    base = np.array([[-30.0, -30.0], [-30.0, 30.0], [30.0, 30.0], [30.0, -30.0]]) @ np.array([[c, s], [-s, c]])
    ext = np.abs(base).max()
    rng = np.random.default_rng(1)
    frames, quads, kinds = [], [], []
    for poke, kind in ((-1.5, "inside"), (10.0, "poking"), (ext, "half")):
        for centre in ((ext - poke, 80.0), (w - 1 - ext + poke, 80.0), (100.0, ext - poke), (100.0, h - 1 - ext + poke)):
            true = base + centre
            frames.append(render_quad(w, h, true))
            quads.append([(true + rng.uniform(-1, 1, (4, 2))).astype(np.float32)])
            kinds.append(kind)
    frames, quads = np.stack(frames), np.array(quads, np.float32)
    want = qn.refine(frames, quads)
    dropped = [r[0]["notes"]["dropped"] for r in want]
    print("dropped stations (two passes):", dict(zip(range(len(kinds)), zip(kinds, dropped))))
    for kind, r in zip(kinds, want):
        assert r[0]["status"] == (qn.WEAK if kind == "half" else qn.OK)
        assert (r[0]["notes"]["dropped"] > 0) == (kind != "inside")
    got = device_refine(torch_cuda, frames, quads)
    assert np.array_equal(got[0]["status"][:, 0], [r[0]["status"] for r in want])
    compare(got, want, quads)


def test_bad_quads_are_refused_by_value_and_leave_their_neighbours_alone(torch_cuda):
    seq = ts.sequence("small")
    front = ts.front_tags(seq, 0)
    good = ts.quads(seq, 0, noise=1.0, seed=SEED)[front]
    sq = np.array([[100.0, 100.0], [100.0, 140.0], [140.0, 140.0], [140.0, 100.0]], np.float32)
    bad = []
    for value in (np.nan, np.inf, -np.inf, float(2 ** 21), -1e30):
        for slot in range(8):
            q = sq.copy(); q.reshape(-1)[slot] = value
            bad.append(q)
    bad += [np.full((4, 2), np.nan, np.float32), sq[[0, 2, 1, 3]], np.array([[100, 100], [120, 120], [140, 140], [140, 100]], np.float32),
            np.repeat(sq[:1], 4, axis=0), np.zeros((4, 2), np.float32)]
    n_degenerate = len(bad)
    bad += [np.array([[100.0, 100.0], [100.0, 107.9], [140.0, 140.0], [140.0, 100.0]], np.float32), sq[::-1] * np.float32(0.19)]
    # interleaved: bad, good, bad, good ... so that every workgroup holds both
    quads, is_bad = [], []
    for i, q in enumerate(bad):
        quads += [q, good[i % len(good)]]
        is_bad += [i, -1]
    quads, is_bad = np.stack(quads)[None], np.array(is_bad)
    frames = seq.frame(0)[None]
    got = device_refine(torch_cuda, frames, quads)
    st = got[0]["status"][0]
    assert np.all(st[(is_bad >= 0) & (is_bad < n_degenerate)] == qn.DEGENERATE) and np.all(st[is_bad >= n_degenerate] == qn.SHORT), st
    assert np.all(st[is_bad < 0] == qn.OK)
    alone = device_refine(torch_cuda, frames, good[None])
    for i in np.nonzero(is_bad < 0)[0]:
        j = (i // 2) % len(good)
        assert got[2][0, i].tobytes() == alone[2][0, j].tobytes() and got[0][0, i].tobytes() == alone[0][0, j].tobytes()
    compare(got, qn.refine(frames, quads), quads)
    assert n_degenerate == 45


def test_both_orientations(torch_cuda):
    seq = ts.sequence("small")
    front = ts.front_tags(seq, 0)
    q = ts.quads(seq, 0, noise=1.0, seed=SEED)[front]
    quads = np.concatenate([q, q[:, ::-1]])[None]
    got = device_refine(torch_cuda, seq.frame(0)[None], quads)
    assert np.all(got[0]["status"] == qn.OK)
    n = len(front)
    assert np.abs(got[2][0, :n] - got[2][0, n:, ::-1]).max() <= TOL
    compare(got, qn.refine(seq.frame(0)[None], quads), quads)


@pytest.mark.parametrize("kw", [dict(iters=1), dict(iters=8), dict(range_px=0.5), dict(range_px=16.0), dict(iters=3, range_px=1.0, min_strength=150.0)])
def test_options(torch_cuda, kw):
    seq = ts.sequence("c2" if kw.get("range_px") == 16.0 else "small")
    frames = seq.frame(0)[None]
    quads = ts.quads(seq, 0, noise=min(1.0, kw.get("range_px", 2.0)), seed=SEED)[None]
    got = device_refine(torch_cuda, frames, quads, **kw)
    print(kw, "status", got[0]["status"][0], "passes", got[0]["passes"][0])
    assert np.all(got[0]["passes"][0][got[0]["status"][0] == qn.OK] == kw.get("iters", 2))
    compare(got, qn.refine(frames, quads, **kw), quads, min_strength=kw.get("min_strength", 40.0))


def test_two_runs_are_bitwise_equal(torch_cuda):
    seq = ts.sequence("dense")
    frames = seq.frame(0)[None]
    quads = np.concatenate([ts.quads(seq, 0, noise=1.0, seed=SEED), ts.background_quads(seq, 64)])[None]
    a, b = device_refine(torch_cuda, frames, quads), device_refine(torch_cuda, frames, quads)
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()


def test_cv_refine_quads_equals_refine_quads(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    seq = ts.sequence("small")
    quads = np.concatenate([ts.quads(seq, 0, noise=1.0, seed=SEED), ts.background_quads(seq, 8)])
    out, rec = cv_hip.refineQuads(seq.frame(0), quads, rangePx=2.0, iters=2, minStrength=40.0)
    got = device_refine(torch_cuda, seq.frame(0)[None], quads[None])
    assert out.dtype == np.float32 and out.tobytes() == got[1][0].tobytes() and rec.tobytes() == got[0][0].tobytes()
    assert set(rec["status"]) == {qn.OK, qn.WEAK}
    out, rec = cv_hip.refineQuads(seq.frame(0), np.zeros((0, 4, 2)))
    assert out.shape == (0, 4, 2) and rec.shape == (0,) and rec.dtype == qn.RECORD_DTYPE
    with pytest.raises(cv_hip.error):
        cv_hip.refineQuads(seq.frame(0).astype(np.float32), quads)
    with pytest.raises(cv_hip.error):
        cv_hip.refineQuads(seq.frame(0), quads[:, :3])
    with pytest.raises(cv_hip.error, match="AGT_QUADFIT_ERR_ARG"):
        cv_hip.refineQuads(seq.frame(0), quads, iters=9)


def test_refined_quads_decode_to_their_ids(torch_cuda):
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import quad_refine, tag_decode
    seq = ts.sequence("small")
    family = tag_decode.TagFamily(ts.family_codes(), "synthetic36")
    frames = torch.from_numpy(seq.frame(0)[None]).cuda()
    ref = quad_refine.refine_quads(frames, torch.from_numpy(ts.quads(seq, 0, noise=1.0, seed=SEED)[None]).cuda())
    dec = tag_decode.decode_quads(frames, ref.quads, family, mask=ref.ok, expected=torch.arange(len(seq.obj) // 4, dtype=torch.int32, device="cuda"))
    torch.cuda.synchronize()
    rec, front = tag_decode.records_numpy(dec.records)[0], ts.front_tags(seq, 0)
    assert np.array_equal(rec["id"][front], front) and np.all(rec["status"][front] == 0) and np.all(rec["rot"][front] == 0)
    assert np.all(dec.ok.cpu().numpy()[0, front] == 1)


def test_tracker_refine_tags(torch_cuda):
    """after reset with corners 1 px off refine_tags equals refine_quads on the same buffer; a tag with a lost corner is MASKED; the
    result is accepted by step_detected and its pose is closer to the scene's than the one the noised corners give"""
    torch = torch_cuda
    from accurate_aprilgroup_tracking_amd import hiplib as H, quad_refine
    from accurate_aprilgroup_tracking_amd.tracker import StreamTracker
    seq = ts.sequence("small")
    T = len(seq.obj) // 4
    front = ts.front_tags(seq, 0)
    noised = ts.quads(seq, 0, noise=1.0, seed=SEED).reshape(1, 4 * T, 2)
    frame = torch.from_numpy(seq.frame(0)[None]).cuda().contiguous()
    corners = torch.from_numpy(noised).cuda().contiguous()
    trk = StreamTracker(seq.width, seq.height, seq.obj, seq.K, seq.dist, n_streams=1)
    trk.reset(frame, corners)
    records, refined, cmask = trk.refine_tags(frame)
    want = quad_refine.refine_quads(frame, corners.view(1, T, 4, 2))
    torch.cuda.synchronize()
    assert refined.shape == (1, trk.n, 2) and refined.dtype == torch.float32 and refined.is_contiguous() and cmask.shape == (1, trk.n)
    assert records.cpu().numpy().tobytes() == want.records.cpu().numpy().tobytes()
    assert refined.cpu().numpy().tobytes() == want.quads.cpu().numpy().tobytes() and torch.equal(cmask, want.corner_mask)
    rec = quad_refine.records_numpy(records)[0]
    assert np.all(rec["status"][front] == qn.OK)

    def translation_error(state):
        return float(np.linalg.norm(state[H.ST_TVEC:H.ST_TVEC + 3] - seq.tvecs[0]))
    # the pose of the noised corners against the pose of the refined ones, every front tag used in both
    use = np.zeros((1, T, 4), np.uint8); use[0, front] = 1
    use = torch.from_numpy(use.reshape(1, trk.n)).cuda()
    s_noised, s_refined = trk.new_state_buffer(), trk.new_state_buffer()
    trk.estimate_pose(corners, use, s_noised)
    trk.step_detected(frame, refined, cmask & use, s_refined)
    torch.cuda.synchronize()
    s_noised, s_refined = s_noised.cpu().numpy()[0], s_refined.cpu().numpy()[0]
    e_noised, e_refined = translation_error(s_noised), translation_error(s_refined)
    print("translation error: noised corners %.5f m, refined corners %.5f m" % (e_noised, e_refined))
    assert s_noised[H.ST_OK] == 1.0 and s_refined[H.ST_OK] == 1.0
    assert e_refined < e_noised

    # a tag with one lost corner is not fitted
    lost = int(front[1])
    status = torch.ones((1, trk.n), dtype=torch.uint8, device="cuda")
    status[0, 4 * lost + 2] = 0
    trk.step_detected(frame, corners, status)
    records, refined, cmask = trk.refine_tags(frame)
    torch.cuda.synchronize()
    rec, cm = quad_refine.records_numpy(records)[0], cmask.cpu().numpy()[0].reshape(T, 4)
    assert rec["status"][lost] == qn.MASKED and not cm[lost].any()
    others = [t for t in front if t != lost]
    assert np.all(rec["status"][others] == qn.OK) and np.all(cm[others] == 1)
    assert refined.cpu().numpy()[0, 4 * lost:4 * lost + 4].tobytes() == noised[0, 4 * lost:4 * lost + 4].tobytes()
