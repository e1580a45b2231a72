"""CPU: the exact statement of the pose operations (tests/pose_exact.py, mpmath) and the table made from it
(tests/golden/pose_range.npz), which tests/test_gpu_pose_range.py holds the device code to.

  * the table regenerates bit for bit (where mpmath is installed);
  * the two float64 statements of the projection -- tests/pnp_numpy.py and the C oracle -- agree with it to 8 eps of a block's
    scale on the rungs where OpenCV's form does not cancel (theta = 0, 5e-3 <= theta <= 7); measured: up to 6.9 eps (the rotation
    block at theta = 1e-2), 1 eps on the pinhole camera;
  * their distance from exact is printed on EVERY rung (profiles/pose_range.md keeps the table): at small angles 1 - cos(theta)
    cancels in OpenCV's dR/dr table, which is why the GPU tests need the exact statement;
  * the scenes of the GPU tests do what they are for: every rung of the matrix-to-vector ladder keeps a factor of two from the
    1e-5 rule, the oracle's matrix-to-vector code is within the pose bound of the exact logarithm on the theta = pi rungs, the
    state-machine scenes cross the identity / the half turn with every frame accepted.
"""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(HERE, "golden"))

import pnp_numpy                       # noqa: E402
import pose_range_scenes as prs        # noqa: E402
from pose_range_scenes import block_ratios, pixel_ratios      # noqa: E402

EPS = float(np.finfo(np.float64).eps)
CAMS = ("pinhole", "mild", "tilt14")
FOCAL = prs.FOCAL


@pytest.fixture(scope="module")
def table():
    return dict(np.load(os.path.join(HERE, "golden", "pose_range.npz")))


def test_table_regenerates_bit_for_bit(table):
    pytest.importorskip("mpmath")
    import make_pose_range_fixture as mk
    import pose_exact as E
    from accurate_aprilgroup_tracking_amd import synthetic
    import calib_scenes
    assert np.array_equal(E.MILD_DIST, synthetic.MILD_DIST.ravel()) and np.array_equal(E.TILT14, calib_scenes.TILT14)
    fresh = mk.tables()
    assert sorted(fresh) == sorted(table)
    for k, v in fresh.items():
        assert v.dtype == table[k].dtype and v.shape == table[k].shape and v.tobytes() == table[k].tobytes(), k
    assert os.path.getsize(mk.PATH) < 256 * 1024


def test_float64_statements_against_exact(table, oracle):
    """prints the table of profiles/pose_range.md; asserts 8 eps where nothing cancels"""
    theta, pose, obj = table["theta"], table["pose"], table["obj"]
    Kmat = table["K"]
    assert Kmat[0, 0] == FOCAL == Kmat[1, 1]
    dists = {"pinhole": None, "mild": table["dist_mild"], "tilt14": table["dist_tilt14"]}
    worst = {}
    for cam in CAMS:
        for b in range(len(theta)):
            for name in ("numpy", "oracle"):
                if name == "numpy":
                    px, J = pnp_numpy.project(obj[b], pose[b, :3], pose[b, 3:], Kmat, dists[cam], jacobian=True)
                else:
                    px, J = oracle.projectPoints(obj[b], pose[b, :3], pose[b, 3:], Kmat, dists[cam], jacobian=True)
                    px = px.reshape(-1, 2)
                rp = pixel_ratios(px, table["px_" + cam][b]).max()
                rj = block_ratios(J.reshape(6, 2, 6), table["jac_" + cam][b]).max(axis=0)
                w = worst.setdefault(float(theta[b]), np.zeros(3))
                worst[float(theta[b])] = np.maximum(w, [rp, rj[0], rj[1]])
                if theta[b] == 0.0 or 5e-3 <= theta[b] <= 7.0:
                    assert max(rp, rj[0], rj[1]) <= 8 * EPS, (cam, name, theta[b], rp / EPS, rj / EPS)
    print("\nfloat64 statements (pnp_numpy, oracle) against exact, worst over axes, cameras and points, in units of eps of the block scale")
    print("%-24s %12s %14s %14s" % ("theta", "pixels", "rotation block", "translation"))
    for t in sorted(worst):
        print("%-24.17g %12.3g %14.3g %14.3g" % (t, *(worst[t] / EPS)))


def test_matrix_to_vector_ladder(table, oracle):
    older, newer, kind = table["inv_older"], table["inv_newer"], table["inv_kind"]
    assert not older[:, :3].any()
    phi = 2.0 * np.linalg.norm(newer[:, :3], axis=1)
    s, c = np.abs(np.sin(phi)), np.cos(phi)
    # a factor of two from the 1e-5 rule on |sin| on either side (sin(2e-5) is 2e-5 less 7e-11 of itself: taken to 1e-9)
    assert ((s <= 0.5e-5) | (s >= 2e-5 * (1 - 1e-9))).all()
    want = np.where(s > 1e-5, 2, np.where(c > 0, 0, 1))
    assert np.array_equal(kind, want) and (kind == 0).sum() == 2 and (kind == 1).sum() == 18 and (kind == 2).sum() == 6
    # the oracle on the theta = pi rungs: its distance from the exact logarithm, up to the sign of the whole vector at pi itself
    print()
    worst = 0.0
    for m in np.flatnonzero(kind == 1):
        r = oracle.Rodrigues(table["inv_Rp"][m])[0].ravel()
        x = table["inv_log"][m]
        d = min(np.abs(r - x).max(), np.abs(r + x).max() + (np.pi - np.linalg.norm(x)))
        print("pi rung %2d: phi - pi = %+.3g, |oracle - exact log| = %.3g" % (m, phi[m] - np.pi, d))
        worst = max(worst, d)
    print("the square roots of (R_ii + 1) / 2 cost the oracle %.3g of the vector near a coordinate axis" % worst)
    # exact log and exact rotation are inverse to each other, and |log| <= pi
    assert (np.linalg.norm(table["inv_log"], axis=1) <= np.pi).all()
    for m in range(len(kind)):
        R = prs.rotation(table["inv_log"][m])
        assert np.abs(R - table["inv_Rp"][m]).max() <= 8 * EPS


@pytest.mark.parametrize("variant", ["identity", "pi"])
def test_state_machine_scenes(oracle, variant):
    sc = prs.TurnScene(variant)
    rec = prs.mirror_run(sc)
    assert rec["pose_valid"].all(), "every frame is accepted"
    truth = np.concatenate([sc.rvecs, sc.tvecs], axis=1)
    err = np.abs(rec["pose"] - truth)
    # (through pi the solver may answer with the other name of a rotation: compared as rotations)
    dR = max(np.abs(prs.rotation(p[:3]) - prs.rotation(q[:3])).max() for p, q in zip(rec["pose"], truth))
    print("\n%s: mirror against truth, rotation matrices %.3g, translation %.3g; guesses %d, sign changes of the guess %d; n_vel %s"
          % (variant, dR, err[:, 3:].max(), rec["guess_valid"].sum(), prs.guess_sign_changes(rec), rec["n_vel"].tolist()))
    assert dR < 1e-6 and err[:, 3:].max() < 1e-6
    assert rec["guess_valid"].all() and rec["n_vel"][-1] == 2
    assert prs.guess_sign_changes(rec) == 1
    if variant == "pi":
        # the half turn lies between two frames: the rotation angle of the accepted poses is within 2 degrees of pi on both sides
        ang = np.linalg.norm(rec["pose"][:, :3], axis=1)
        assert (np.abs(ang[6:8] - np.pi) < np.deg2rad(prs.STEP_DEG)).all() and ang[6] < np.pi
