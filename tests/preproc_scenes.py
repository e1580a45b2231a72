"""Small named scenes for the pre-processing kernels (csrc/agt_preproc.hip), shared by the CPU and GPU halves of
tests/test_preproc_edges.py.  A scene is a source size, a camera (K, dist, newK), a list of ROIs (rx, ry, rw, rh) and B frames of noise;
its maps and expected outputs come from tests/preproc_numpy.py, are computed once and never modified.

  windows        300 x 80, a mild lens seen far off-axis: ROI widths around the 4-pixel group and the 256-pixel segment, ROI heights around
                 the 8-row band and the 8-band (64-row) XCD split, origins 0..3 (group alignment against the map and the destination)
  shift-*        64 x 24, pure translations by multiples of 1/32 px: sx on -2 .. 1 and sw-4 .. sw, sy on -2 .. 0 and sh-2 .. sh
  tiny-WxH       frames smaller than a group, a tap or a band
  sat            map values beyond int32 (saturated: they sample real pixels)
  wrap_home      map values beyond int16 whose wrapped entry lands back in the source
  wrap_far       map values beyond int16 whose wrapped entry does not
  full14         the 14-coefficient tilted lens with an off-centre ROI
  wide257        a 257-pixel row: the second block of the one-pixel-per-thread BGR kernel
"""
import numpy as np

from accurate_aprilgroup_tracking_amd import synthetic as syn

import preproc_numpy

# the full 14-coefficient model: rational radial, tangential, thin prism and a TILTED sensor (tau_x, tau_y in radians)
TILTED_DIST = np.array([[0.05, -0.02, 1e-3, 2e-3, 0.01, 0.02, -0.01, 0.005, 1e-3, -2e-3, 5e-4, 1e-3, 0.03, -0.02]])
SAT_DIST = np.array([[0.4, 0.3, 0.01, -0.02, 0.1]])


def bgr(h, w, seed):
    """smooth noise stretched to the full 8-bit range, three independent channels"""
    rng = np.random.default_rng(seed)
    from scipy.ndimage import gaussian_filter
    img = np.stack([gaussian_filter(rng.standard_normal((h, w)), 1.2) for _ in range(3)], axis=-1)
    img = (img - img.min()) / (img.max() - img.min()) * 255
    return img.astype(np.uint8)


def _frames(w, h, B, seed):
    if min(w, h) < 8:           # (too small to smooth and stretch: plain bytes)
        return np.random.default_rng(seed).integers(0, 256, size=(B, h, w, 3), dtype=np.uint8)
    return np.stack([bgr(h, w, seed * 100 + b) for b in range(B)])


class Scene:
    def __init__(self, name, w, h, K, dist, newK, rois, B=3):
        self.name, self.w, self.h, self.B = name, w, h, B
        self.K = np.asarray(K, np.float64); self.newK = np.asarray(newK, np.float64)
        self.dist = None if dist is None else np.asarray(dist, np.float64)
        self.rois = list(rois)
        for rx, ry, rw, rh in self.rois:
            assert 0 <= rx and 0 <= ry and rw >= 1 and rh >= 1 and rx + rw <= w and ry + rh <= h
        self._frames = self._maps = self._remapped = None
        self._ref = {}

    @property
    def frames(self):
        """u8 [B, h, w, 3], a different image per batch entry"""
        if self._frames is None:
            self._frames = _frames(self.w, self.h, self.B, sum(map(ord, self.name)))
            self._frames.setflags(write=False)
        return self._frames

    @property
    def maps(self):
        """the numpy statement's (map1 i16 [h, w, 2], map2 u16 [h, w])"""
        if self._maps is None:
            self._maps = preproc_numpy.undistort_maps(self.K, self.dist, self.newK, self.w, self.h)
            for m in self._maps:
                m.setflags(write=False)
        return self._maps

    @property
    def remapped(self):
        """the numpy statement's cv.undistort of every frame: u8 [B, h, w, 3]"""
        if self._remapped is None:
            self._remapped = np.stack([preproc_numpy.remap(f, *self.maps) for f in self.frames])
            self._remapped.setflags(write=False)
        return self._remapped

    def expected(self, roi, undistort=True):
        """the numpy statement's agt_preprocess_bgr output: u8 [B, rh, rw]"""
        key = (tuple(roi), bool(undistort))
        if key not in self._ref:
            rx, ry, rw, rh = roi
            src = self.remapped if undistort else self.frames
            r = np.ascontiguousarray(preproc_numpy.gray(src)[:, ry:ry + rh, rx:rx + rw])
            r.setflags(write=False)
            self._ref[key] = r
        return self._ref[key]

    def modes(self):
        """undistort flags: every scene also runs without undistortion (gray + crop only; the maps play no part)"""
        return (True, False)

    def class_counts(self, base4):
        """classify() summed over the scene's ROIs"""
        tot = dict.fromkeys(preproc_numpy.CLASSES, 0)
        for roi in self.rois:
            for k, v in preproc_numpy.class_counts(self.maps[0], roi, self.w, self.h, base4).items():
                tot[k] += v
        return tot


def _K(f, cx, cy):
    return np.array([[f, 0.0, cx], [0.0, f, cy], [0.0, 0.0, 1.0]])


K96 = syn.camera_matrix(96, 40)
K96[0, 2] += 0.3; K96[1, 2] -= 0.2

# (rx, ry, rw, rh): every rw of {1 2 3 4 5 7 8 255 256 257 260}, rx of {0 1 2 3}, rh of {1 7 8 9 63 64 65 72 73}, ry of {0 1 5} at
# least once -- wide ones with every rh and rx (the band split, the segment edge), narrow ones (tails only) likewise
WINDOWS = [(0, 0, 260, 73), (1, 1, 257, 72), (3, 5, 256, 65), (2, 0, 255, 64), (0, 5, 256, 63), (1, 0, 257, 9), (2, 1, 260, 8), (3, 0, 255, 7),
           (0, 1, 256, 1), (3, 0, 260, 64), (1, 5, 255, 65), (2, 1, 257, 73),
           (0, 0, 1, 1), (1, 1, 2, 7), (2, 5, 3, 8), (3, 0, 4, 9), (0, 1, 5, 63), (1, 5, 7, 64), (2, 0, 8, 65), (3, 1, 1, 72), (0, 5, 2, 73),
           (1, 0, 3, 1), (2, 1, 4, 64), (3, 5, 5, 8), (0, 0, 7, 9), (1, 1, 8, 7)]
# The mild lens with newK = K is the identity near the principal point, and the windows end at column 262 of 300: a camera whose
# principal point sits at the left (focal 100, c = (40.3, 39.8)) stretches the right half, so the map crosses the last source columns
# -- sw - 3, sw - 2 -- inside the windows, and leaves the source on all four sides.
K_WINDOWS = _K(100.0, 40.3, 39.8)

SW, SH = 64, 24
K_SHIFT = _K(75.0, 32.0, 12.0)
# u = j + tx, v = i + ty: (tx, ty) in 1/32 px, all with non-zero fractions
SHIFTS = {
    "shift-lt": (-55 / 32, 13 / 32),      # sx -2 .. 61 (-2 -1 0 1 sw-4 sw-3), sy 0 .. 23 (0 sh-2 sh-1): the entries at (sx <= 1, sy = 0)
    "shift-rb": (42 / 32, 51 / 32),       # sx 1 .. 64 (sw-2 sw-1 sw), sy 1 .. 24 (sh)
    "shift-lu": (-55 / 32, -58 / 32),     # sy -2 .. 21 (-2 -1)
    "shift-ru": (42 / 32, -26 / 32),      # sx 1 .. 64, sy -1 .. 22
    "shift-in": (8 / 32, 16 / 32),        # sx 0 .. 63, sy 0 .. 23
}
SHIFT_ROIS = [(0, 0, 64, 24), (1, 0, 63, 24), (2, 0, 62, 24), (2, 1, 61, 22), (3, 2, 58, 9), (0, 0, 6, 24), (57, 15, 7, 9)]
TINY = {(1, 1): (9 / 32, 13 / 32), (2, 2): (-9 / 32, 13 / 32), (3, 3): (9 / 32, -13 / 32), (4, 2): (-23 / 32, 5 / 32), (5, 1): (17 / 32, -7 / 32),
        (8, 4): (21 / 32, 11 / 32)}


def _shifted(K, tx, ty):
    n = K.copy(); n[0, 2] -= tx; n[1, 2] -= ty
    return n


SCENES = {}


def _add(sc):
    SCENES[sc.name] = sc


_add(Scene("windows", 300, 80, K_WINDOWS, syn.MILD_DIST, K_WINDOWS, WINDOWS))
for _n, (_tx, _ty) in SHIFTS.items():
    _add(Scene(_n, SW, SH, K_SHIFT, np.zeros(5), _shifted(K_SHIFT, _tx, _ty), SHIFT_ROIS))
for (_w, _h), (_tx, _ty) in TINY.items():
    _Kt = _K(75.0, _w / 2, _h / 2)
    _add(Scene("tiny-%dx%d" % (_w, _h), _w, _h, _Kt, np.zeros(5), _shifted(_Kt, _tx, _ty), [(0, 0, _w, _h)]))
_add(Scene("sat", 96, 40, K96, SAT_DIST, _K(2.0, 48.0, 20.0), [(0, 0, 96, 40), (3, 2, 90, 37)]))
_add(Scene("wrap_home", 96, 40, K96, np.zeros(5), np.array([[75 / 8192, 0.0, 40.0], [0.0, 75.0, 20.0], [0.0, 0.0, 1.0]]),
           [(0, 0, 96, 40), (1, 3, 94, 33)]))
_add(Scene("wrap_far", 96, 40, K96, SAT_DIST, _K(6.0, 48.0, 20.0), [(0, 0, 96, 40), (2, 1, 93, 38)]))
_add(Scene("full14", 96, 40, K96, TILTED_DIST, K96, [(9, 3, 70, 30), (0, 0, 96, 40)]))
_add(Scene("wide257", 257, 9, _K(100.0, 40.3, 4.2), syn.MILD_DIST, _K(100.0, 40.3, 4.2), [(0, 0, 257, 9), (1, 1, 256, 8)]))

SHIFT_NAMES = list(SHIFTS)
TINY_NAMES = [n for n in SCENES if n.startswith("tiny")]
GUARD_SCENE = "shift-lt"            # map entries at (sx <= 1, sy = 0): what an unaligned frame must keep off the aligned-load path
