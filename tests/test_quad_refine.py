"""CPU: the quad edge refinement library (include/agt_quadfit.h -> libagt_quadfit.so) builds, exports exactly its header, keeps its
kernel out of scratch and LDS and judges its arguments without a device; the numpy statement of the rule (tests/quad_refine_numpy.py)
that the GPU tests compare with finds the rendered corners, tells a tag's border from background and has the properties the rule
promises."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import quad_refine_numpy as qn     # noqa: E402
import tag_decode_scenes as ts     # noqa: E402

NOISE, SEED = 1.0, 3


def test_quadfit_library_builds_exports_and_resources():
    import side_library
    from accurate_aprilgroup_tracking_amd import quadfitlib
    rows = side_library.built(quadfitlib, "quadfit")
    assert [re.search(r"(quad_\w+)\(", r["name"]).group(1) for r in rows] == ["quad_refine_kernel"]
    print(rows[0])
    # no private segment, no LDS, and room for four waves per SIMD
    bad = [(r["name"], r["scratch"], r["vgpr"], r["vspill"], r["sspill"], r["lds"]) for r in rows
           if r["scratch"] != 0 or r["vgpr"] > 128 or r["vspill"] != 0 or r["sspill"] != 0 or r["lds"] != 0]
    assert not bad, bad
    assert quadfitlib.lib().agt_quadfit_version() == quadfitlib.VERSION == 100
    assert quadfitlib.RECORD_DTYPE == qn.RECORD_DTYPE
    assert (quadfitlib.MAX_COORD, quadfitlib.MIN_EDGE) == (qn.MAX_COORD, qn.MIN_EDGE) and quadfitlib.STATUS_NAMES == qn.STATUS_NAMES


def test_argument_errors_need_no_device():
    """no pointer is followed: every refusal comes before device work.  (A call with good arguments would launch: none is made.)"""
    from accurate_aprilgroup_tracking_amd import quadfitlib as Q
    L = Q.lib()
    good = dict(frames=64, pitch=640, frame_stride=640 * 480, width=640, height=480, B=2, quads=64, Q=12, range_px=2.0, iters=2, min_strength=40.0,
                quads_out=64, records=64)

    def refine(**kw):
        a = dict(good, **kw)
        return L.agt_quad_refine(None, a["frames"], a["pitch"], a["frame_stride"], a["width"], a["height"], a["B"], a["quads"], None, a["Q"],
                                 a["range_px"], a["iters"], a["min_strength"], a["quads_out"], None, a["records"], None, None)
    for k in ("frames", "quads", "quads_out", "records"):
        assert refine(**{k: None}) == Q.ERR_ARG, k
    for kw in (dict(width=3), dict(height=3), dict(width=Q.MAX_SIZE + 1, pitch=1 << 20, frame_stride=1 << 40), dict(height=Q.MAX_SIZE + 1, frame_stride=1 << 40),
               dict(pitch=639), dict(frame_stride=640 * 479 + 639), dict(B=0), dict(Q=0), dict(B=-1), dict(B=1 << 10, Q=(1 << 10) + 1),
               dict(B=1 << 16, Q=1 << 16), dict(range_px=0.0), dict(range_px=-1.0), dict(range_px=16.5), dict(range_px=float("nan")),
               dict(range_px=float("inf")), dict(iters=0), dict(iters=9), dict(iters=-1), dict(min_strength=-1.0), dict(min_strength=float("nan")),
               dict(min_strength=float("inf"))):
        assert refine(**kw) == Q.ERR_ARG, kw
    with pytest.raises(Q.QuadFitError, match="AGT_QUADFIT_ERR_ARG"):
        Q.refine(None, 64, 640, 640 * 480, 640, 480, 1, 64, None, 12, 2.0, 0, 40.0, 64, None, 64, None, None)


def test_missing_library_raises(monkeypatch):
    from accurate_aprilgroup_tracking_amd import quadfitlib
    monkeypatch.setattr(quadfitlib, "_lib", None)
    monkeypatch.setattr(quadfitlib, "LIB_PATH", "/nonexistent/libagt_quadfit.so")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        quadfitlib.lib()


def corner_errors(res, truth):
    return np.array([np.linalg.norm(r["quad64"] - t, axis=1) for r, t in zip(res, truth)])


@pytest.mark.parametrize("name", ["c2", "dense", "small"])
def test_numpy_statement_finds_the_rendered_corners(name):
    """frame 0, every tag seen at under 60 degrees, seeds 1 px off: all OK, and as close to the truth as the issue's table asks"""
    seq = ts.sequence(name)
    front = ts.front_tags(seq, 0)
    assert len(front) >= 8
    truth, seeds = ts.quads(seq, 0).astype(np.float64)[front], ts.quads(seq, 0, noise=NOISE, seed=SEED)[front]
    res = [qn.refine_quad(seq.frame(0), q, range_px=2.0, iters=2) for q in seeds]
    err_in, err = corner_errors([dict(quad64=q.astype(np.float64)) for q in seeds], truth), corner_errors(res, truth)
    clean = corner_errors([qn.refine_quad(seq.frame(0), q) for q in ts.quads(seq, 0)[front]], truth)
    strength = min(r["strength"] for r in res)
    print("%s: %d tags, edges %.0f-%.0f px, seed error max %.3f, refined max %.3f median %.3f (from exact seeds: max %.3f median %.3f), "
          "smallest strength %.1f, largest resid %.3f" % (name, len(front), ts.smallest_edge(truth), np.linalg.norm(np.roll(truth, -1, axis=1) - truth, axis=2).max(),
                                                         err_in.max(), err.max(), np.median(err), clean.max(), np.median(clean), strength, max(r["resid"] for r in res)))
    assert [r["status"] for r in res] == [qn.OK] * len(front) and all(r["passes"] == 2 and r["ok"] == 1 for r in res)
    if name == "small":
        assert err.max() <= 0.5 and np.median(err) <= 0.25
    else:
        assert err.max() < 0.25 * err_in.max() and err.max() < 0.35
    assert strength >= 80.0
    assert all(np.array_equal(r["quad"], r["quad64"].astype(np.float32)) for r in res)


@pytest.mark.parametrize("name", ["c2", "dense", "small"])
def test_numpy_statement_refuses_bare_background(name):
    seq = ts.sequence(name)
    bg = ts.background_quads(seq, 40)
    res = [qn.refine_quad(ts.bare_frame(seq), q) for q in bg]
    print("%s: status counts %s, largest strength %.2f" % (name, np.bincount([r["status"] for r in res], minlength=6), max(r["strength"] for r in res)))
    assert all(r["status"] == qn.WEAK and r["ok"] == 0 for r in res)
    assert all(r["quad"].tobytes() == q.tobytes() and np.array_equal(r["quad64"], q.astype(np.float64)) for r, q in zip(res, bg))


def test_reversed_quad_gives_the_reversed_result():
    seq = ts.sequence("small")
    q = ts.quads(seq, 0, noise=NOISE, seed=SEED)
    for i in ts.front_tags(seq, 0)[:6]:
        a, b = qn.refine_quad(seq.frame(0), q[i]), qn.refine_quad(seq.frame(0), q[i][::-1])
        assert a["status"] == b["status"] == qn.OK
        assert np.abs(a["quad64"] - b["quad64"][::-1]).max() <= 1e-12
        assert abs(a["strength"] - b["strength"]) <= 1e-12 and abs(a["shift"] - b["shift"]) <= 1e-12


def test_whole_pixel_shift_of_frame_and_quad_shifts_the_result():
    seq = ts.sequence("small")
    frame = seq.frame(0)
    q = np.round(ts.quads(seq, 0, noise=NOISE, seed=SEED) * 64) / 64         # (f32 holds the moved seeds exactly as well)
    sx, sy = 7, 5
    moved = np.zeros((seq.height + sy, seq.width + sx), np.uint8)
    moved[sy:, sx:] = frame
    for i in ts.front_tags(seq, 0)[:6]:
        a, b = qn.refine_quad(frame, q[i]), qn.refine_quad(moved, q[i] + np.float32([sx, sy]))
        assert a["status"] == b["status"] == qn.OK
        assert np.abs(b["quad64"] - a["quad64"] - [sx, sy]).max() <= 1e-10
        assert abs(a["strength"] - b["strength"]) <= 1e-10


def test_a_third_pass_hardly_moves_the_corners():
    seq = ts.sequence("c2")
    q = ts.quads(seq, 0, noise=NOISE, seed=SEED)
    moves = []
    for i in ts.front_tags(seq, 0):
        a, b = qn.refine_quad(seq.frame(0), q[i], iters=2), qn.refine_quad(seq.frame(0), q[i], iters=3)
        assert a["status"] == b["status"] == qn.OK and b["passes"] == 3
        moves.append(np.linalg.norm(a["quad64"] - b["quad64"], axis=1).max())
    print("iters 3 against iters 2 on c2: largest move %.4f px" % max(moves))
    assert max(moves) < 0.05


def test_seeds_beyond_the_search_range_are_right_or_refused():
    """3 px of noise on tags whose edges are 11..19 px (L / 8 under 2.4 px): OK within 2 range_px of the seed, or untouched"""
    seq = ts.sequence("small")
    q = ts.quads(seq, 0, noise=3.0, seed=SEED)
    res = [qn.refine_quad(seq.frame(0), q[i]) for i in ts.front_tags(seq, 0)]
    print("noise 3 on small: status counts %s" % np.bincount([r["status"] for r in res], minlength=6))
    for r, i in zip(res, ts.front_tags(seq, 0)):
        if r["status"] == qn.OK:
            assert np.linalg.norm(r["quad64"] - q[i].astype(np.float64), axis=1).max() <= 2 * 2.0 and r["shift"] <= 2 * 2.0
        else:
            assert r["quad"].tobytes() == q[i].tobytes() and r["ok"] == 0


def test_refusals_by_value_follow_the_precedence():
    seq = ts.sequence("small")
    frame = seq.frame(0)
    sq = np.array([[100.0, 100.0], [100.0, 140.0], [140.0, 140.0], [140.0, 100.0]], np.float32)
    for bad in (np.nan, np.inf, -np.inf, float(2 ** 21), -float(2 ** 21)):
        for slot in range(8):
            q = sq.copy(); q.reshape(-1)[slot] = bad
            r = qn.refine_quad(frame, q)
            assert r["status"] == qn.DEGENERATE and r["quad"].tobytes() == q.tobytes()
            assert (r["passes"], r["strength"], r["shift"], r["resid"]) == (0, 0.0, 0.0, 0.0)
    bowtie, collinear = sq[[0, 2, 1, 3]], np.array([[100, 100], [120, 120], [140, 140], [140, 100]], np.float32)
    for q in (bowtie, collinear, np.repeat(sq[:1], 4, axis=0), np.zeros((4, 2), np.float32)):
        assert qn.refine_quad(frame, q)["status"] == qn.DEGENERATE
    short = np.array([[100.0, 100.0], [100.0, 107.9], [140.0, 140.0], [140.0, 100.0]], np.float32)
    assert qn.refine_quad(frame, short)["status"] == qn.SHORT
    assert qn.refine_quad(frame, short[::-1])["status"] == qn.SHORT
    eight = np.array([[100.0, 100.0], [100.0, 108.0], [108.0, 108.0], [108.0, 100.0]], np.float32)
    assert qn.refine_quad(frame, eight)["status"] not in (qn.SHORT, qn.DEGENERATE)
    # a short AND bow-tie quad is DEGENERATE; anything masked is MASKED
    assert qn.refine_quad(frame, np.array([[0, 0], [4, 4], [4, 0], [0, 4]], np.float32))["status"] == qn.DEGENERATE
    for q in (sq, bowtie, short, np.full((4, 2), np.nan, np.float32)):
        r = qn.refine_quad(frame, q, masked=True)
        assert r["status"] == qn.MASKED and r["quad"].tobytes() == q.tobytes() and r["ok"] == 0
    # a quad far outside the frame: every station dropped -> WEAK, corners untouched
    far = sq + np.float32(5000.0)
    r = qn.refine_quad(frame, far)
    assert r["status"] == qn.WEAK and r["strength"] == 0.0 and r["quad"].tobytes() == far.tobytes()


@pytest.mark.parametrize("name", ["small", "dense", "c2"])
def test_gpu_parity_inputs_stay_clear_of_the_decisions(name):
    """the GPU parity tests may leave out no tag quad: with the seeds used there the numpy statement shows every decision (strength
    against min_strength, sample points against the frame limit, station sums against zero) further than 1e-6 from flipping"""
    seq = ts.sequence(name)
    for k in ((0, 1) if name == "small" else (0,)):
        for noise in ((0.0, 1.0, 2.0) if name == "small" else (1.0,)):
            for r in (qn.refine_quad(seq.frame(k), q) for q in ts.quads(seq, k, noise=noise, seed=SEED)):
                if r["status"] in (qn.OK, qn.WEAK, qn.DIVERGED):
                    assert abs(r["strength"] - 40.0) > 1e-6 and r["notes"]["frame_limit"] > 1e-6 and r["notes"]["Mc"] > 1e-6
