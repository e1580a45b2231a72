"""Pre-processing (csrc/agt_preproc.hip: the map build, cv.undistort to BGR, the fused undistort + gray + crop kernel; entries
agt_undistort_init / agt_undistort_maps / agt_undistort_bgr / agt_preprocess_bgr) at the windows, alignments and map ranges the workload
never reaches: ROIs narrower than a 4-pixel group, at the 256-pixel segment edge and on both sides of a band edge, destinations and
sources at every byte alignment and with odd pitches, taps on the first and last columns and rows, frames smaller than a group, map
values beyond int16 and beyond int32, and the bytes next to the ROI.

Three implementations of one specification: tests/preproc_numpy.py (the reference of this file), the C oracle and the HIP kernels, on
the scenes of tests/preproc_scenes.py.  Everything is integer after the map formula and compared BIT-EXACT: no tolerance anywhere.  The
CPU half holds the oracle to the numpy statement on every scene and asserts that each scene reaches what it is built to reach; the GPU
half holds the kernels to the statement, and every destination is pre-filled with a sentinel that must survive outside the ROI (pitch
padding, rows after the ROI, the gap between batch entries).  Sources sit in 0xFF: a byte taken from outside the frame shows.
"""
import ctypes as C

import numpy as np
import pytest

import preproc_numpy
import preproc_scenes
from preproc_scenes import SCENES, SHIFT_NAMES, GUARD_SCENE

ALL = list(SCENES)
SENT = 0xA5             # destination sentinel
SURROUND = 0xFF         # what lies around a source frame
MARGIN = 16             # bytes of sentinel / surround before and after every buffer's payload
ERR_ARG, ERR_STATE = -1, -7


# --------------------------------------------------------------------------- CPU half
@pytest.mark.parametrize("name", ALL)
def test_oracle_equals_numpy_statement(oracle, name):
    """the oracle's maps, its cv.undistort (BGR and one channel) and undistort -> crop -> cvtColor against the numpy statement"""
    sc = SCENES[name]
    size = (sc.w, sc.h)
    o1, o2 = oracle.initUndistortRectifyMap(sc.K, sc.dist, sc.newK, size)
    n1, n2 = sc.maps
    assert np.array_equal(o1, n1) and np.array_equal(o2, n2), "%d map entries differ" % ((o1 != n1).any(-1) | (o2 != n2)).sum()
    for b in range(sc.B):
        f = sc.frames[b]
        und = oracle.undistort(f, sc.K, sc.dist, None, sc.newK)
        assert np.array_equal(und, sc.remapped[b])
        g = np.ascontiguousarray(f[..., 1])
        assert np.array_equal(oracle.undistort(g, sc.K, sc.dist, None, sc.newK), preproc_numpy.remap(g, n1, n2))
        for roi in sc.rois:
            rx, ry, rw, rh = roi
            for on in sc.modes():
                full = und if on else f
                ref = oracle.cvtColor(np.ascontiguousarray(full[ry:ry + rh, rx:rx + rw]), oracle.COLOR_BGR2GRAY)
                mine = preproc_numpy.preprocess(f, n1, n2, roi, on)
                assert mine.shape == (rh, rw) and mine.dtype == np.uint8
                assert np.array_equal(ref, mine) and np.array_equal(mine, sc.expected(roi, on)[b])


@pytest.mark.parametrize("name", ALL)
def test_map_formula_is_finite(name):
    """the kernel and the oracle are not asked to agree on NaN or infinity: no scene produces one"""
    sc = SCENES[name]
    with np.errstate(all="raise"):
        f = preproc_numpy.map_formula(sc.K, sc.dist, sc.newK, sc.w, sc.h)
    for k, v in f.items():
        assert np.isfinite(v).all(), k


def _tap_in(m1, sw, sh):
    sx, sy = m1[..., 0].astype(np.int64), m1[..., 1].astype(np.int64)
    return (sx >= -1) & (sx <= sw - 1) & (sy >= -1) & (sy <= sh - 1)


@pytest.mark.parametrize("base4", [True, False])
def test_windows_and_shift_reach_every_class(base4):
    """windows: interior, inside, partial and tail groups; the shift scenes: those and outside groups -- for an aligned frame
    and for an unaligned one (whose groups at sx <= 1, sy = 0 leave the interior class)"""
    w = SCENES["windows"].class_counts(base4)
    print("windows base4=%s %s" % (base4, w))
    for c in ("interior", "inside", "partial", "tail"):
        assert w[c] > 0, c
    tot = dict.fromkeys(preproc_numpy.CLASSES, 0)
    for n in SHIFT_NAMES:
        cc = SCENES[n].class_counts(base4)
        print("%s base4=%s %s" % (n, base4, cc))
        for k, v in cc.items():
            tot[k] += v
    for c in preproc_numpy.CLASSES:
        assert tot[c] > 0, c


def test_windows_use_every_value():
    rois = SCENES["windows"].rois
    assert {r[2] for r in rois} == {1, 2, 3, 4, 5, 7, 8, 255, 256, 257, 260} and {r[0] for r in rois} == {0, 1, 2, 3}
    assert {r[3] for r in rois} == {1, 7, 8, 9, 63, 64, 65, 72, 73} and {r[1] for r in rois} == {0, 1, 5}
    # every height and origin with a wide window (bands, segments) and with a narrow one (tails only)
    for wide in (True, False):
        sel = [r for r in rois if (r[2] >= 255) == wide]
        assert {r[3] for r in sel} == {1, 7, 8, 9, 63, 64, 65, 72, 73} and {r[0] for r in sel} == {0, 1, 2, 3}


def test_shift_puts_entries_on_every_edge_value():
    sxs, sys_ = set(), set()
    for n in SHIFT_NAMES:
        sc = SCENES[n]
        m1, m2 = sc.maps
        assert (m2 & 31).all() and (m2 >> 5).all(), "fractions must be non-zero"
        assert (np.diff(m1[..., 0].astype(int), axis=1) == 1).all() and (np.diff(m1[..., 1].astype(int), axis=0) == 1).all()
        sxs |= set(m1[0, :, 0].tolist()); sys_ |= set(m1[:, 0, 1].tolist())
    sw, sh = preproc_scenes.SW, preproc_scenes.SH
    assert {-2, -1, 0, 1, sw - 4, sw - 3, sw - 2, sw - 1, sw} <= sxs and {-2, -1, 0, sh - 2, sh - 1, sh} <= sys_
    m1 = SCENES[GUARD_SCENE].maps[0]
    guard = ((m1[..., 0] >= 0) & (m1[..., 0] <= 1) & (m1[..., 1] == 0)).sum()
    assert guard >= 2
    # ... and they decide the class of a whole-frame group only when the frame is unaligned
    roi = (2, 0, 62, 24)
    assert roi in SCENES[GUARD_SCENE].rois
    a = preproc_numpy.classify(m1, roi, sw, sh, True); b = preproc_numpy.classify(m1, roi, sw, sh, False)
    assert a[0, 0] == "interior" and b[0, 0] == "inside" and (a[1:] == b[1:]).all()


def test_sat_scene_saturates_onto_real_pixels():
    sc = SCENES["sat"]
    f = preproc_numpy.map_formula(sc.K, sc.dist, sc.newK, sc.w, sc.h)
    beyond = (np.abs(f["us"]) >= 2.0 ** 31) | (np.abs(f["vs"]) >= 2.0 ** 31)
    n = int((beyond & _tap_in(sc.maps[0], sc.w, sc.h)).sum())
    nz = int((sc.expected((0, 0, sc.w, sc.h))[0] != 0).sum())
    print("sat: %d of %d entries beyond int32 with a tap in the source; %d non-zero output pixels" % (n, beyond.size, nz))
    assert n >= 1000 and nz >= 1000


def test_wrap_scenes_wrap_home_and_far():
    sc = SCENES["wrap_home"]
    f = preproc_numpy.map_formula(sc.K, sc.dist, sc.newK, sc.w, sc.h)
    beyond = (np.abs(f["u"]) >= 32768) | (np.abs(f["v"]) >= 32768)
    n = int((beyond & _tap_in(sc.maps[0], sc.w, sc.h)).sum())
    print("wrap_home: %d wrapped entries with a tap in the source" % n)
    assert n >= 200
    assert (np.abs(f["us"]) < 2.0 ** 31).all() and (np.abs(f["vs"]) < 2.0 ** 31).all()      # wrapped, not saturated
    sc = SCENES["wrap_far"]
    f = preproc_numpy.map_formula(sc.K, sc.dist, sc.newK, sc.w, sc.h)
    beyond = (np.abs(f["u"]) >= 32768) | (np.abs(f["v"]) >= 32768)
    home = int((beyond & _tap_in(sc.maps[0], sc.w, sc.h)).sum())
    print("wrap_far: %d wrapped entries, %d with a tap in the source" % (beyond.sum(), home))
    assert beyond.sum() > 0 and home == 0


def test_classify_on_a_hand_made_map():
    """classify() itself, on entries written by hand (source 16 x 6)"""
    sw, sh = 16, 6
    m1 = np.zeros((1, 22, 2), np.int16)
    m1[0, 0:4, 0] = [2, 3, 4, 12]                  # interior: 12 = sw - 4
    m1[0, 4:8, 0] = [2, 3, 4, 13]                  # 13 = sw - 3: inside
    m1[0, 8:12, 0] = [0, 1, 2, 3]                  # sy = 0, sx <= 1: interior only when base4
    m1[0, 12:16, 0] = [13, 14, 15, 16]             # taps in and out: partial
    m1[0, 16:20, 0] = [16, 17, -2, -3]             # outside
    m1[0, 20:22, 0] = [5, 6]                       # tail
    assert preproc_numpy.classify(m1, (0, 0, 22, 1), sw, sh, True)[0].tolist() == ["interior", "inside", "interior", "partial", "outside", "tail"]
    assert preproc_numpy.classify(m1, (0, 0, 22, 1), sw, sh, False)[0].tolist() == ["interior", "inside", "inside", "partial", "outside", "tail"]
    m1[0, :, 1] = sh - 1                           # the lower taps leave: nothing is all in
    assert preproc_numpy.classify(m1, (0, 0, 20, 1), sw, sh, True)[0].tolist() == ["partial", "partial", "partial", "partial", "outside"]
    m1[0, :, 1] = 1
    assert preproc_numpy.classify(m1, (8, 0, 4, 1), sw, sh, False)[0].tolist() == ["interior"]      # sy > 0 lifts the guard
    m1[0, :, 1] = sh
    assert (preproc_numpy.classify(m1, (0, 0, 20, 1), sw, sh, True) == "outside").all()


# --------------------------------------------------------------------------- GPU half
@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a ROCm device"
    return torch


class _Rig:
    """one context; the scene whose maps it holds; uploaded frames"""

    def __init__(self, torch):
        from accurate_aprilgroup_tracking_amd import cv_hip
        self.torch = torch
        self.ctx = cv_hip.Context(64, 64, max_level=0)
        self.L, self.h = self.ctx.L, self.ctx.h
        self.current = None
        self.dev = {}

    def use(self, sc):
        if self.current != sc.name:
            self.ctx.undistort_init(sc.K, sc.dist, sc.newK, sc.w, sc.h)
            self.current = sc.name

    def frames(self, sc):
        """cuda u8 [B, h, w, 3], contiguous"""
        if sc.name not in self.dev:
            self.dev[sc.name] = self.torch.from_numpy(np.array(sc.frames)).cuda()
        return self.dev[sc.name]


@pytest.fixture(scope="module")
def rig(torch_cuda):
    return _Rig(torch_cuda)


class _Dst:
    """a sentinel-filled device allocation with B x rows x rowbytes payload bytes at (off, pitch, batch) inside it"""

    def __init__(self, torch, B, rows, rowbytes, off=0, pitch=None, batch=None):
        self.pitch = rowbytes if pitch is None else pitch
        self.batch = self.pitch * rows if batch is None else batch
        assert self.pitch >= rowbytes and self.batch >= self.pitch * rows
        self.shape, self.off = (B, rows, rowbytes), MARGIN + off
        self.n = self.off + (B - 1) * self.batch + (rows - 1) * self.pitch + rowbytes + MARGIN
        self.buf = torch.full((self.n,), SENT, dtype=torch.uint8, device="cuda")

    @property
    def ptr(self):
        return self.buf.data_ptr() + self.off

    def view(self):
        """the payload as a strided tensor (what Context.preprocess_bgr takes as out=)"""
        return self.buf.as_strided(self.shape, (self.batch, self.pitch, 1), self.off)

    def _payload(self, a):
        return np.lib.stride_tricks.as_strided(a[self.off:], self.shape, (self.batch, self.pitch, 1), writeable=True)

    def check(self, expected, what):
        got = self.buf.cpu().numpy()
        pay = self._payload(got)
        bad = pay != expected
        assert not bad.any(), "%s: %d of %d payload bytes differ, first at (b, row, byte) %s" % (what, bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))
        want = np.full(self.n, SENT, np.uint8)
        self._payload(want)[...] = expected
        stray = np.flatnonzero(got != want)
        assert stray.size == 0, "%s: %d bytes outside the payload were written, first at offset %d of the payload" % (what, stray.size, stray[0] - self.off)

    def check_untouched(self, what):
        assert bool((self.buf == SENT).all()), "%s: the destination was written" % what


class _Src:
    """frames u8 [B, h, w, 3] inside a device allocation of SURROUND bytes at (off, pitch, batch)"""

    def __init__(self, torch, frames, off=0, pitch=None, batch=None):
        B, h, w, _ = frames.shape
        self.pitch = 3 * w if pitch is None else pitch
        self.batch = self.pitch * h if batch is None else batch
        assert self.pitch >= 3 * w and self.batch >= self.pitch * h
        o = MARGIN + off
        host = np.full(o + (B - 1) * self.batch + (h - 1) * self.pitch + 3 * w + MARGIN, SURROUND, np.uint8)
        np.lib.stride_tricks.as_strided(host[o:], (B, h, 3 * w), (self.batch, self.pitch, 1), writeable=True)[...] = frames.reshape(B, h, 3 * w)
        self.buf = torch.from_numpy(host).cuda()
        self.ptr = self.buf.data_ptr() + o
        self.B, self.h, self.w = B, h, w


def _abi_gray(rig, src, roi, undistort, dst, B=None):
    rx, ry, rw, rh = roi
    return rig.L.agt_preprocess_bgr(rig.h, C.c_void_p(src.ptr), src.pitch, src.batch, src.w, src.h, src.B if B is None else B, int(undistort),
                                    rx, ry, rw, rh, C.c_void_p(dst.ptr), dst.pitch, dst.batch)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_hip_maps_equal_numpy_statement(rig, name):
    sc = SCENES[name]
    rig.current = None
    rig.use(sc)
    m1, m2 = rig.ctx.undistort_maps()
    n1, n2 = sc.maps
    bad = (m1 != n1).any(-1) | (m2 != n2)
    assert m1.shape == n1.shape and m2.shape == n2.shape and not bad.any(), "%d of %d map entries differ, first at (row, col) %s" % (
        bad.sum(), bad.size, tuple(np.argwhere(bad)[0]))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ALL)
def test_hip_fused_gray_equals_numpy_statement(rig, name):
    """Context.preprocess_bgr over every ROI of the scene, B = 1 and the scene's B, with and without undistortion: ROI bytes equal,
    everything else of a pitch-padded, gap-separated destination untouched"""
    torch = rig.torch
    sc = SCENES[name]
    rig.use(sc)
    frames = rig.frames(sc)
    for roi in sc.rois:
        rx, ry, rw, rh = roi
        for on in sc.modes():
            for B in sorted({1, sc.B}):
                d = _Dst(torch, B, rh, rw, pitch=(rw + 15) & ~15, batch=((rw + 15) & ~15) * rh + 48)
                out = rig.ctx.preprocess_bgr(frames[:B], roi, undistort=on, out=d.view())
                assert out.data_ptr() == d.ptr
                d.check(sc.expected(roi, on)[:B], "%s roi %s undistort %s B %d" % (name, roi, on, B))
    # the wrapper's own destination (pitch padded to 16)
    roi = sc.rois[0]
    assert np.array_equal(rig.ctx.preprocess_bgr(frames, roi).cpu().numpy(), sc.expected(roi))


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["windows"] + SHIFT_NAMES)
def test_hip_fused_gray_at_every_destination_alignment(rig, name):
    """destination views with base offset 0 .. 3 and the odd pitch rw + 5: the byte-store and the dword-store branch on the same
    pixels (a row's alignment changes from row to row)"""
    torch = rig.torch
    sc = SCENES[name]
    rig.use(sc)
    frames = rig.frames(sc)
    for roi in sc.rois:
        rx, ry, rw, rh = roi
        for on in sc.modes():
            for off in range(4):
                d = _Dst(torch, sc.B, rh, rw, off=off, pitch=rw + 5, batch=(rw + 5) * rh + 7)
                assert d.ptr % 4 == off
                rig.ctx.preprocess_bgr(frames, roi, undistort=on, out=d.view())
                d.check(sc.expected(roi, on), "%s roi %s undistort %s destination offset %d" % (name, roi, on, off))


@pytest.mark.gpu
@pytest.mark.parametrize("on", [True, False])
@pytest.mark.parametrize("name", [GUARD_SCENE, "sat"])
def test_hip_fused_gray_at_every_source_alignment(rig, name, on):
    """the frames inside a larger buffer of 0xFF at base offsets 0 .. 3 with pitches 3 w .. 3 w + 3, through the C ABI (the Python
    wrapper takes contiguous frames only), on the scenes with map entries at (sx <= 1, sy = 0) -- the translation, and the saturated
    map whose whole groups sit on (0, 0): only offset 0 with pitch 3 w (a multiple of 4 here) may take the aligned loads for those"""
    torch = rig.torch
    sc = SCENES[name]
    m1 = sc.maps[0]
    assert any((preproc_numpy.classify(m1, r, sc.w, sc.h, True) != preproc_numpy.classify(m1, r, sc.w, sc.h, False)).any() for r in sc.rois)
    assert (3 * sc.w) % 4 == 0
    rig.use(sc)
    for off in range(4):
        for extra in range(4):
            src = _Src(torch, sc.frames, off=off, pitch=3 * sc.w + extra, batch=(3 * sc.w + extra) * sc.h + 5 + off)
            assert src.ptr % 4 == off
            for roi in sc.rois:
                rx, ry, rw, rh = roi
                d = _Dst(torch, sc.B, rh, rw, pitch=rw + 3)
                assert _abi_gray(rig, src, roi, on, d) == 0
                d.check(sc.expected(roi, on), "roi %s undistort %s source offset %d pitch 3w+%d" % (roi, on, off, extra))


@pytest.mark.gpu
@pytest.mark.parametrize("name", SHIFT_NAMES + ["sat", "wrap_home", "wide257"])
def test_hip_undistort_bgr_equals_numpy_statement(rig, name):
    """agt_undistort_bgr (one pixel per thread) on contiguous and on pitch-padded, gap-separated buffers, B = 3"""
    torch = rig.torch
    sc = SCENES[name]
    rig.use(sc)
    w, h, B = sc.w, sc.h, sc.B
    assert B == 3
    want = sc.remapped.reshape(B, h, 3 * w)
    for (soff, sextra, sgap), (doff, dextra, dgap) in (((0, 0, 0), (0, 0, 0)), ((1, 5, 9), (3, 7, 11)), ((2, 2, 0), (1, 0, 5))):
        src = _Src(torch, sc.frames, off=soff, pitch=3 * w + sextra, batch=(3 * w + sextra) * h + sgap)
        d = _Dst(torch, B, h, 3 * w, off=doff, pitch=3 * w + dextra, batch=(3 * w + dextra) * h + dgap)
        assert rig.L.agt_undistort_bgr(rig.h, C.c_void_p(src.ptr), src.pitch, src.batch, C.c_void_p(d.ptr), d.pitch, d.batch, B) == 0
        d.check(want, "%s source (off, pitch+, gap) %s destination %s" % (name, (soff, sextra, sgap), (doff, dextra, dgap)))
    assert np.array_equal(rig.ctx.undistort_bgr(rig.frames(sc)).cpu().numpy(), sc.remapped)
    # refusals: a pitch below the row, no frames
    src = _Src(torch, sc.frames); d = _Dst(torch, B, h, 3 * w)
    for args in ((3 * w - 1, src.batch, d.pitch, d.batch, B), (src.pitch, src.batch, 3 * w - 1, d.batch, B), (src.pitch, src.batch, d.pitch, d.batch, 0)):
        assert rig.L.agt_undistort_bgr(rig.h, C.c_void_p(src.ptr), args[0], args[1], C.c_void_p(d.ptr), args[2], args[3], args[4]) == ERR_ARG
    d.check_untouched("refused agt_undistort_bgr")


@pytest.mark.gpu
def test_hip_cv_undistort_of_a_gray_frame_with_saturated_maps(torch_cuda):
    from accurate_aprilgroup_tracking_amd import cv_hip
    sc = SCENES["sat"]
    g = np.ascontiguousarray(sc.frames[0][..., 1])
    want = preproc_numpy.remap(g, *sc.maps)
    assert (want != 0).sum() >= 1000
    assert np.array_equal(cv_hip.undistort(g, sc.K, sc.dist, None, sc.newK), want)
    assert np.array_equal(cv_hip.undistort(np.array(sc.frames[0]), sc.K, sc.dist, None, sc.newK), sc.remapped[0])


@pytest.mark.gpu
def test_hip_fused_gray_batch_of_300_with_gaps(rig):
    """300 frames of 16 x 8 (gridDim.y far beyond one wave of workgroups), every frame different, source and destination batch
    strides larger than a frame"""
    torch = rig.torch
    w, h, B = 16, 8, 300
    K = np.array([[75.0, 0.0, 8.0], [0.0, 75.0, 4.0], [0.0, 0.0, 1.0]])
    newK = K.copy(); newK[0, 2] -= 11 / 32; newK[1, 2] += 7 / 32
    frames = np.random.default_rng(300).integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)
    m1, m2 = preproc_numpy.undistort_maps(K, np.zeros(5), newK, w, h)
    rig.ctx.undistort_init(K, np.zeros(5), newK, w, h)
    rig.current = None
    src = _Src(torch, frames, off=1, pitch=3 * w + 1, batch=(3 * w + 1) * h + 13)
    for roi in ((0, 0, w, h), (1, 1, 14, 7)):
        for on in (True, False):
            want = np.stack([preproc_numpy.preprocess(f, m1, m2, roi, on) for f in frames])
            assert len({r.tobytes() for r in want}) == B
            d = _Dst(torch, B, roi[3], roi[2], off=2, pitch=roi[2] + 3, batch=(roi[2] + 3) * roi[3] + 9)
            assert _abi_gray(rig, src, roi, on, d) == 0
            d.check(want, "300 frames roi %s undistort %s" % (roi, on))


@pytest.mark.gpu
def test_hip_map_lifetime_reuse_reallocate_and_size_check(torch_cuda):
    """undistort_init twice at one size (the buffers are reused), then another size (reallocated), then the first again: after each
    step the fused kernel follows the camera set last, and frames of another size than the maps are refused with AGT_ERR_STATE"""
    rig = _Rig(torch_cuda)
    torch = torch_cuda
    a, b, c = SCENES["shift-lt"], SCENES["shift-rb"], SCENES["sat"]
    assert (a.w, a.h) == (b.w, b.h) != (c.w, c.h) and not np.array_equal(a.maps[0], b.maps[0])
    other = {a.name: c, b.name: c, c.name: a}
    for sc in (a, b, c, a, c, b):
        rig.use(sc)
        m1, m2 = rig.ctx.undistort_maps()
        assert np.array_equal(m1, sc.maps[0]) and np.array_equal(m2, sc.maps[1])
        for roi in sc.rois:
            d = _Dst(torch, sc.B, roi[3], roi[2], pitch=roi[2] + 1)
            rig.ctx.preprocess_bgr(rig.frames(sc), roi, out=d.view())
            d.check(sc.expected(roi), "after undistort_init(%s): roi %s" % (sc.name, roi))
        # frames of the other size: refused with the maps in place, accepted without undistortion
        o = other[sc.name]
        src = _Src(torch, o.frames)
        d = _Dst(torch, o.B, o.h, o.w)
        assert _abi_gray(rig, src, (0, 0, o.w, o.h), True, d) == ERR_STATE
        d.check_untouched("frames of another size than the maps")
        assert _abi_gray(rig, src, (0, 0, o.w, o.h), False, d) == 0
        d.check(o.expected((0, 0, o.w, o.h), False), "gray only, frames of another size than the maps")
    # a context without maps
    fresh = _Rig(torch_cuda)
    src = _Src(torch, a.frames); d = _Dst(torch, a.B, a.h, a.w)
    assert _abi_gray(fresh, src, (0, 0, a.w, a.h), True, d) == ERR_STATE
    assert fresh.L.agt_undistort_bgr(fresh.h, C.c_void_p(src.ptr), src.pitch, src.batch, C.c_void_p(d.ptr), 3 * a.w, 3 * a.w * a.h, 1) == ERR_STATE
    d.check_untouched("a context without maps")
    fresh.ctx.close(); rig.ctx.close()


@pytest.mark.gpu
def test_hip_refusals_leave_the_destination_alone(rig):
    """AGT_ERR_ARG before anything is launched: ROI outside the source (four ways), empty ROI, pitches below a row, B = 0; and
    agt_undistort_init with a width beyond int16 or a singular new camera matrix -- after which the maps set before still hold"""
    torch = rig.torch
    sc = SCENES["shift-in"]
    rig.use(sc)
    w, h = sc.w, sc.h
    src = _Src(torch, sc.frames)
    d = _Dst(torch, sc.B, h, w)
    for roi in ((-1, 0, 8, 8), (0, -1, 8, 8), (w - 7, 0, 8, 8), (0, h - 7, 8, 8), (0, 0, w + 1, h), (0, 0, w, h + 1),
                (0, 0, 0, 8), (0, 0, 8, 0), (0, 0, -4, 8), (0, 0, 8, -4)):
        for on in (True, False):
            assert _abi_gray(rig, src, roi, on, d) == ERR_ARG, roi
    for on in (True, False):
        assert _abi_gray(rig, src, (0, 0, w, h), on, d, B=0) == ERR_ARG
        assert _abi_gray(rig, src, (0, 0, w, h), on, d, B=-1) == ERR_ARG
        rx, ry, rw, rh = 0, 0, w, h
        assert rig.L.agt_preprocess_bgr(rig.h, C.c_void_p(src.ptr), 3 * w - 1, src.batch, w, h, sc.B, int(on), rx, ry, rw, rh,
                                        C.c_void_p(d.ptr), d.pitch, d.batch) == ERR_ARG
        assert rig.L.agt_preprocess_bgr(rig.h, C.c_void_p(src.ptr), src.pitch, src.batch, w, h, sc.B, int(on), rx, ry, rw, rh,
                                        C.c_void_p(d.ptr), rw - 1, d.batch) == ERR_ARG
        assert rig.L.agt_preprocess_bgr(rig.h, None, src.pitch, src.batch, w, h, sc.B, int(on), rx, ry, rw, rh,
                                        C.c_void_p(d.ptr), d.pitch, d.batch) == ERR_ARG
    d.check_untouched("refused agt_preprocess_bgr")
    K = np.ascontiguousarray(sc.K); nd = np.zeros(5)
    ptr = lambda a: a.ctypes.data_as(C.c_void_p)
    singular = np.array([[75.0, 0.0, 32.0], [0.0, 0.0, 12.0], [0.0, 0.0, 1.0]])
    assert rig.L.agt_undistort_init(rig.h, ptr(K), ptr(nd), 5, ptr(K), 32768, 8) == ERR_ARG
    assert rig.L.agt_undistort_init(rig.h, ptr(K), ptr(nd), 5, ptr(K), 8, 32768) == ERR_ARG
    assert rig.L.agt_undistort_init(rig.h, ptr(K), ptr(nd), 5, ptr(K), 0, 8) == ERR_ARG
    assert rig.L.agt_undistort_init(rig.h, ptr(K), ptr(nd), 5, ptr(singular), w, h) == ERR_ARG
    assert rig.L.agt_undistort_init(rig.h, ptr(K), ptr(nd), 5, ptr(singular), 2 * w, h) == ERR_ARG
    # the refused calls changed nothing: the maps of the scene still serve
    m1, m2 = rig.ctx.undistort_maps()
    assert np.array_equal(m1, sc.maps[0]) and np.array_equal(m2, sc.maps[1])
    assert _abi_gray(rig, src, (0, 0, w, h), True, d) == 0
    d.check(sc.expected((0, 0, w, h)), "after the refusals")
