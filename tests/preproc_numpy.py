"""Frame pre-processing (csrc/agt_preproc.hip; oracle/cv_imgproc.c) as plain numpy: the second statement the oracle and the kernels
are held to, bit for bit.  Integers throughout after the map formula; nothing here is tuned to an implementation.

  undistort_maps   cv::initUndistortRectifyMap(K, dist, I, newK, (w, h), CV_16SC2)
  remap            cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) with those maps on 8-bit images
  gray             cv::cvtColor(COLOR_BGR2GRAY) on 8-bit images (14-bit fixed point)
  preprocess       remap (or not) -> gray -> crop: what agt_preprocess_bgr writes
  classify         which path of the fused gray kernel each 4-pixel output group of an ROI needs (scene fitness only)
"""
import numpy as np

INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1


def map_formula(K, dist, newK, w, h):
    """every intermediate of the map formula, float64 [h, w] each, by name (the order of operations is OpenCV's)"""
    k = np.zeros(14)
    if dist is not None:
        d = np.asarray(dist, np.float64).reshape(-1); k[:d.size] = d
    K = np.asarray(K, np.float64)
    ir = np.linalg.inv(np.asarray(newK, np.float64))
    j, i = np.meshgrid(np.arange(w, dtype=np.float64), np.arange(h, dtype=np.float64))
    _x = j * ir[0, 0] + (i * ir[0, 1] + ir[0, 2]); _y = j * ir[1, 0] + (i * ir[1, 1] + ir[1, 2]); _w = j * ir[2, 0] + (i * ir[2, 1] + ir[2, 2])
    x, y = _x * (1.0 / _w), _y * (1.0 / _w)
    x2, y2 = x * x, y * y
    r2, _2xy = x2 + y2, 2 * x * y
    kr = (1 + ((k[4] * r2 + k[1]) * r2 + k[0]) * r2) / (1 + ((k[7] * r2 + k[6]) * r2 + k[5]) * r2)
    xd = x * kr + k[2] * _2xy + k[3] * (r2 + 2 * x2) + k[8] * r2 + k[9] * r2 * r2
    yd = y * kr + k[2] * (r2 + 2 * y2) + k[3] * _2xy + k[10] * r2 + k[11] * r2 * r2
    if k[12] != 0 or k[13] != 0:        # tilted sensor (tests/pnp_numpy.py tilt_matrix)
        from tests.pnp_numpy import tilt_matrix
        T = tilt_matrix(k[12], k[13])
        hx, hy, hw = (T[q, 0] * xd + T[q, 1] * yd + T[q, 2] for q in range(3))
        xd, yd = hx / hw, hy / hw
    u = K[0, 0] * xd + K[0, 2]; v = K[1, 1] * yd + K[1, 2]
    return dict(x=x, y=y, r2=r2, kr=kr, xd=xd, yd=yd, u=u, v=v, us=u * 32, vs=v * 32)


def undistort_maps(K, dist, newK, w, h):
    """cv::initUndistortRectifyMap(K, dist, I, newK, (w, h), CV_16SC2), vectorised (written from OpenCV's documented model:
    inverse new camera matrix -> normalised point -> Brown-Conrady + thin prism -> pixel -> 1/32-pixel fixed point).  The
    fixed-point value is saturate_cast<int>: rounded half to even and clamped to int32; the int16 cast of the pixel part WRAPS."""
    f = map_formula(K, dist, newK, w, h)
    iu = np.clip(np.rint(f["us"]), INT32_MIN, INT32_MAX).astype(np.int64)
    iv = np.clip(np.rint(f["vs"]), INT32_MIN, INT32_MAX).astype(np.int64)
    m1 = np.stack([iu >> 5, iv >> 5], axis=-1).astype(np.int16)
    m2 = ((iv & 31) * 32 + (iu & 31)).astype(np.uint16)
    return m1, m2


def remap(src, m1, m2):
    """cv::remap(INTER_LINEAR, BORDER_CONSTANT 0) with CV_16SC2 maps on 8-bit images: 15-bit weights from the 5-bit fractions"""
    h, w = src.shape[:2]
    sx, sy = m1[..., 0].astype(np.int64), m1[..., 1].astype(np.int64)
    fx, fy = (m2 & 31).astype(np.int64), (m2 >> 5).astype(np.int64)
    pad = np.zeros((h + 2, w + 2) + src.shape[2:], np.int64); pad[1:-1, 1:-1] = src

    def tap(dy, dx):
        yy, xx = sy + dy, sx + dx
        ok = (yy >= 0) & (yy < h) & (xx >= 0) & (xx < w)
        v = pad[np.clip(yy, -1, h) + 1, np.clip(xx, -1, w) + 1]
        return np.where(ok[..., None] if src.ndim == 3 else ok, v, 0)
    ws = [(32 - fx) * (32 - fy) * 32, fx * (32 - fy) * 32, (32 - fx) * fy * 32, fx * fy * 32]
    if src.ndim == 3:
        ws = [x[..., None] for x in ws]
    acc = tap(0, 0) * ws[0] + tap(0, 1) * ws[1] + tap(1, 0) * ws[2] + tap(1, 1) * ws[3]
    return ((acc + (1 << 14)) >> 15).astype(np.uint8)


def gray(bgr):
    """cv::cvtColor(COLOR_BGR2GRAY), 8 bit: (1868 B + 9617 G + 4899 R + 2^13) >> 14"""
    a = bgr.astype(np.int64)
    return ((a[..., 0] * 1868 + a[..., 1] * 9617 + a[..., 2] * 4899 + (1 << 13)) >> 14).astype(np.uint8)


def preprocess(src_bgr, m1, m2, roi, undistort):
    """src_bgr u8 [h, w, 3] -> u8 [rh, rw]: remap with the maps (when `undistort`), BGR to gray, crop to roi = (rx, ry, rw, rh)"""
    rx, ry, rw, rh = roi
    img = remap(src_bgr, m1, m2) if undistort else src_bgr
    return np.ascontiguousarray(gray(img)[ry:ry + rh, rx:rx + rw])


CLASSES = ("interior", "inside", "partial", "outside", "tail")


def classify(m1, roi, sw, sh, base4):
    """-> [rh, ceil(rw / 4)] array of names from CLASSES: what the map entries of every 4-pixel output group of the ROI (groups start
    at the ROI's left edge) require of the fused gray kernel.
      interior  all four entries have 0 <= sx <= sw - 4 and 0 <= sy <= sh - 2 -- and, when the frame's base address or pitch is not a
                multiple of 4 (`base4` false), sx > 1 or sy > 0
      inside    every tap (sx .. sx + 1, sy .. sy + 1) of all four entries is in the source, but the group is not interior
      partial   some taps are in the source, some are not
      outside   no tap is in the source
      tail      the group has fewer than four pixels"""
    rx, ry, rw, rh = roi
    ng = (rw + 3) // 4
    out = np.empty((rh, ng), dtype="U8")
    sx = np.full((rh, ng * 4), 0, np.int64); sy = sx.copy()
    sx[:, :rw] = m1[ry:ry + rh, rx:rx + rw, 0]; sy[:, :rw] = m1[ry:ry + rh, rx:rx + rw, 1]
    have = np.zeros((rh, ng * 4), bool); have[:, :rw] = True
    sx, sy, have = (a.reshape(rh, ng, 4) for a in (sx, sy, have))
    x_in = [(sx + d >= 0) & (sx + d < sw) for d in (0, 1)]
    y_in = [(sy + d >= 0) & (sy + d < sh) for d in (0, 1)]
    taps = np.stack([x_in[dx] & y_in[dy] for dy in (0, 1) for dx in (0, 1)], axis=-1)       # [rh, ng, 4, 4]
    all_in = (taps.all(-1) | ~have).all(-1)
    none_in = (~taps.any(-1) | ~have).all(-1)
    fast = (sx >= 0) & (sx <= sw - 4) & (sy >= 0) & (sy <= sh - 2)
    if not base4:
        fast &= (sx > 1) | (sy > 0)
    out[:] = "partial"
    out[none_in] = "outside"
    out[all_in] = "inside"
    out[fast.all(-1)] = "interior"
    out[~have.all(-1)] = "tail"
    return out


def class_counts(m1, roi, sw, sh, base4):
    c = classify(m1, roi, sw, sh, base4)
    return {name: int((c == name).sum()) for name in CLASSES}
