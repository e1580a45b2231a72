"""CPU: the host code the side libraries share (csrc/agt_side_math.h: the Levenberg-Marquardt loop, cholesky_solve, the tilt matrices;
csrc/agt_side_frames.h: the rule for a batch of frames) driven without a device by tests/side_math_check.cpp -- a program of its own, built with the host compiler under AddressSanitizer and
UBSan (which also shows that the header needs no HIP) and run as a subprocess."""
import ctypes
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONVERGED, MAX_ITERS, LAMBDA = 1, 2, 3
ERR_ARG, ERR_HIP = -1, -5
NAN, INF = float("nan"), float("inf")
DEFAULTS = dict(max_iters=50, ftol=1e-14, lambda0=1e-3, lambda_up=10.0, lambda_down=0.1, lambda_max=1e12)


@pytest.fixture(scope="module")
def program(tmp_path_factory):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path_factory.mktemp("side_math") / "side_math_check")
    # (-ffp-contract=off: as the libraries' host code is compiled)
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "side_math_check.cpp"), "-o", exe])

    def run(*args):
        p = subprocess.run([exe] + [str(a) for a in args], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout[-4000:]
        return p.stdout
    return run


def lm(program, trials, cost0=4.0, n_residuals=16, **options):
    """-> (rc, steps, commits, report or None, lambdas given to the steps)"""
    out = program("lm", *[repr(options[k]) if k in options else "-" for k in DEFAULTS], repr(cost0), n_residuals, *trials).splitlines()
    rc, steps, commits = (int(v) for v in out[0].split())
    if rc:
        return rc, steps, commits, None, None
    r = out[1].split()
    rep = dict(zip(("iterations", "accepted", "stop", "n_residuals"), map(int, r[:4])),
               **dict(zip(("initial_cost", "final_cost", "rms", "lambda"), map(float.fromhex, r[4:]))))
    return rc, steps, commits, rep, [float.fromhex(v) for v in out[2].split()]


# options, initial cost, trial costs ("u": an unsolved step; the last repeats) -> steps run, trials committed, iterations, accepted, stop,
# final cost, final lambda.  Every expectation is worked out from the rule as agt_group_calib_solve states it; l0, up, down are the defaults.
L0, UP, DOWN = DEFAULTS["lambda0"], DEFAULTS["lambda_up"], DEFAULTS["lambda_down"]
LM_CASES = {
    "initial cost 0": ({}, 0.0, [1.0], 0, 0, 0, 0, CONVERGED, 0.0, L0),
    "max_iters 0": (dict(max_iters=0), 4.0, [1.0], 0, 0, 0, 0, MAX_ITERS, 4.0, L0),
    "unsolved, then accepted": (dict(max_iters=2), 4.0, ["u", 1.0], 2, 1, 2, 1, MAX_ITERS, 1.0, L0 * UP * DOWN),
    "NaN trial cost": (dict(max_iters=1), 4.0, [NAN], 1, 0, 1, 0, MAX_ITERS, 4.0, L0 * UP),
    "equal trial cost": (dict(max_iters=1), 4.0, [4.0], 1, 0, 1, 0, MAX_ITERS, 4.0, L0 * UP),
    "lambda0 0, rejected": (dict(lambda0=0.0, max_iters=1), 4.0, [5.0], 1, 0, 1, 0, MAX_ITERS, 4.0, 1e-6),
    "lambda0 0, rejected twice": (dict(lambda0=0.0, max_iters=2), 4.0, [5.0], 2, 0, 2, 0, MAX_ITERS, 4.0, 1e-6 * UP),
    "lambda0 0, accepted": (dict(lambda0=0.0, max_iters=2), 4.0, [3.0, 2.0], 2, 2, 2, 2, MAX_ITERS, 2.0, 0.0),
    # 1 -> 10 -> 100 -> 1000 (not beyond lambda_max) -> 10000
    "rejections up to lambda_max": (dict(lambda0=1.0, lambda_max=1000.0), 4.0, ["u"], 4, 0, 4, 0, LAMBDA, 4.0, 10000.0),
    # the gain is held to ftol times the cost from BEFORE the step: 1.5 <= 0.5 * 4, though 1.5 > 0.5 * 2.5
    "gain within ftol": (dict(ftol=0.5), 4.0, [2.5, 1.0], 1, 1, 1, 1, CONVERGED, 2.5, L0 * DOWN),
    "gain equal to ftol": (dict(ftol=0.5), 4.0, [2.0, 0.5], 1, 1, 1, 1, CONVERGED, 2.0, L0 * DOWN),
    "second gain within ftol": (dict(ftol=0.5), 4.0, [1.0, 0.75, 0.1], 2, 2, 2, 2, CONVERGED, 0.75, L0 * DOWN * DOWN),
    # ... the next trip finds cost == 0 before it counts an iteration
    "step to cost 0": ({}, 4.0, [0.0, 1.0], 1, 1, 1, 1, CONVERGED, 0.0, L0 * DOWN),
}


@pytest.mark.parametrize("name", list(LM_CASES))
def test_lm_loop(program, name):
    options, cost0, trials, steps, commits, iterations, accepted, stop, cost, lam = LM_CASES[name]
    rc, got_steps, got_commits, rep, lambdas = lm(program, trials, cost0, **options)
    print(name, rep, lambdas)
    assert (rc, got_steps, got_commits) == (0, steps, commits)
    assert rep == dict(iterations=iterations, accepted=accepted, stop=stop, n_residuals=16, initial_cost=cost0, final_cost=cost,
                       rms=math.sqrt(2.0 * cost / 16.0), **{"lambda": lam})
    # every step ran at the damping the step before it left
    if name == "unsolved, then accepted":
        assert lambdas == [L0, L0 * UP]
    if name == "lambda0 0, rejected twice":
        assert lambdas == [0.0, 1e-6]
    if name == "rejections up to lambda_max":
        assert lambdas == [1.0, 10.0, 100.0, 1000.0]


def test_lm_loop_ends_with_a_failing_steps_code_and_no_residuals_give_rms_0(program):
    assert lm(program, [3.0, "f"])[:3] == (ERR_HIP, 2, 1)
    assert lm(program, [1.0], 0.0, 0)[3]["rms"] == 0.0


@pytest.mark.parametrize("option, value, accepted", [
    ("max_iters", 0, True), ("ftol", 0.0, True), ("lambda0", 0.0, True), ("lambda_down", 1.0, True), ("lambda_max", INF, True),
    ("max_iters", -1, False), ("ftol", -1e-300, False), ("ftol", NAN, False), ("lambda0", -1e-300, False), ("lambda0", NAN, False),
    ("lambda_up", 1.0, False), ("lambda_up", 0.5, False), ("lambda_up", NAN, False), ("lambda_down", 0.0, False), ("lambda_down", -0.1, False),
    ("lambda_down", 1.5, False), ("lambda_down", NAN, False), ("lambda_max", 0.0, False), ("lambda_max", -1.0, False), ("lambda_max", NAN, False)])
def test_lm_options(program, option, value, accepted):
    """every option agt_group_calib_solve / agt_camcal_solve refuse, and the edge of each that they take"""
    assert lm(program, [1.0], **{option: value})[0] == (0 if accepted else ERR_ARG)


def cholesky(program, tmp_path, A, b):
    path = tmp_path / "system.bin"
    path.write_bytes(np.int32(len(b)).tobytes() + np.asarray(A, np.float64).tobytes() + np.asarray(b, np.float64).tobytes())
    lines = program("chol", path).split()
    assert len(lines) == 1 + len(b)
    return lines[0] == "ok", np.array([float.fromhex(v) for v in lines[1:]])


@pytest.mark.parametrize("n", [1, 6, 378])
def test_cholesky_solve_against_numpy(program, tmp_path, n):
    """random SPD systems up to the largest reduced system (6 (64 - 1)): the residual ||A x - b|| / (||A|| ||x||) within ten times that of
    numpy.linalg.solve on the same system (the margin the step-parity tests take over a measured floor)"""
    rng = np.random.default_rng(1000 + n)
    G = rng.normal(size=(n, n))
    A = G @ G.T + n * np.eye(n)
    A = 0.5 * (A + A.T)
    b = rng.normal(size=n)
    ok, x = cholesky(program, tmp_path, A, b)

    def residual(v):
        return np.linalg.norm(A @ v - b) / (np.linalg.norm(A, 2) * np.linalg.norm(v))
    ours, ref = residual(x), residual(np.linalg.solve(A, b))
    print("n = %d: residual %.3e, numpy.linalg.solve %.3e" % (n, ours, ref))
    assert ok and ours <= 10.0 * ref


def test_cholesky_solve_refusals(program, tmp_path):
    """a zero pivot, a negative one, a NaN or infinite entry (the lower triangle is what it reads)"""
    for A in ([[0.0]], [[-1.0]], [[NAN]], [[INF]], [[1, 0], [1, 1]], [[1, 0], [2, 1]], [[1, 0], [NAN, 1]], [[1, 0, 0], [0, 1, 0], [0, 0, NAN]]):
        assert not cholesky(program, tmp_path, A, np.ones(len(A)))[0], A
    ok, x = cholesky(program, tmp_path, [[4, NAN], [2, 5]], [2, 5])         # L = [2 0; 1 2]
    assert ok and x.tolist() == [0.0, 1.0]


@pytest.mark.parametrize("tau", [(0.0, 0.0), (0.03, -0.02), (1.2, -0.9)])
def test_tilt_matrices_against_the_oracle(program, oracle, tau):
    """matTilt | invMatTilt against cvo_tilt_matrices, at the bound test_oracle.py holds the oracle's to the numpy statement with"""
    M, Mi = np.zeros(9), np.zeros(9)
    oracle.lib().cvo_tilt_matrices(ctypes.c_double(tau[0]), ctypes.c_double(tau[1]), M.ctypes.data_as(ctypes.c_void_p), Mi.ctypes.data_as(ctypes.c_void_p))
    m = np.array([float.fromhex(v) for v in program("tilt", repr(tau[0]), repr(tau[1])).split()])
    assert m.shape == (18,)
    err = max(np.abs(m[:9] - M).max(), np.abs(m[9:] - Mi).max())
    print("tau %s: largest difference %.3e" % (tau, err))
    assert err < 1e-15


# ---- agt_side::frames_ok: one case per clause of the rule.  A library in the style of the quad finder: sizes 8 .. 640 x 480, up to 4
# frames, one byte a pixel; every case changes one thing about a batch that is accepted.
INT_MAX = 2 ** 31 - 1
FRAMES = dict(p=1, pitch=100, stride=0, w=100, h=50, channels=1, B=1, min_size=8, max_w=640, max_h=480, max_B=4)
FRAMES_CASES = [
    ("as it is", {}, True),
    ("null pointer", dict(p=0), False),
    ("width min - 1", dict(w=7, pitch=7), False), ("width min", dict(w=8, pitch=8), True),
    ("width max", dict(w=640, pitch=640), True), ("width max + 1", dict(w=641, pitch=641), False),
    ("height min - 1", dict(h=7), False), ("height min", dict(h=8), True),
    ("height max", dict(h=480), True), ("height max + 1", dict(h=481), False),
    ("pitch row - 1", dict(pitch=99), False), ("pitch row", dict(pitch=100), True), ("pitch beyond the row", dict(pitch=128), True),
    ("B 0", dict(B=0), False), ("B 1, frame_stride 0", dict(B=1, stride=0), True), ("B -1", dict(B=-1), False),
    ("B max_B", dict(B=4, stride=5000), True), ("B max_B + 1", dict(B=5, stride=5000), False),
    ("no cap, B INT_MAX", dict(B=INT_MAX, max_B=INT_MAX, stride=5000), True),
    # the second frame may begin where the last row of the first ends: pitch (h - 1) + row = 128 * 49 + 100
    ("B 2, frames touching", dict(B=2, pitch=128, stride=128 * 49 + 100), True),
    ("B 2, one byte less", dict(B=2, pitch=128, stride=128 * 49 + 100 - 1), False),
    ("B 2, frame_stride 0", dict(B=2, stride=0), False),
    # three bytes a pixel: the row is 300 bytes.  The pitch and the stride that pass for one channel must not
    ("3 channels, pitch of 1 channel", dict(channels=3, pitch=100), False), ("3 channels, pitch row", dict(channels=3, pitch=300), True),
    ("1 channel, stride for 1 channel", dict(B=2, pitch=300, stride=300 * 49 + 100), True),
    ("3 channels, stride for 1 channel", dict(B=2, channels=3, pitch=300, stride=300 * 49 + 100), False),
    ("3 channels, frames touching", dict(B=2, channels=3, pitch=300, stride=300 * 49 + 300), True),
    ("3 channels, one byte less", dict(B=2, channels=3, pitch=300, stride=300 * 49 + 300 - 1), False),
]


@pytest.mark.parametrize("name, change, accepted", FRAMES_CASES, ids=[c[0] for c in FRAMES_CASES])
def test_frames_ok(program, name, change, accepted):
    args = dict(FRAMES, **change)
    assert program("frames", *[args[k] for k in FRAMES]).split() == ["1" if accepted else "0"]
