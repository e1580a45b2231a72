"""Host-side mirror of the reference's `Draw` (aprilgroup_pose_estimation/draw.py:10-194): the same methods issuing the same sequence
of circle and line calls, through `self.cv` -- by default the HIP-backed `cv_hip` module, whose circle and line follow the integer rule
of include/agt_draw.h; cv2 itself serves as well.  Text (putText, the tag id of draw_corners) and filled contours (draw_contours) are
not part of this project.

For frames that live on the device use overlay.draw_pose / StreamTracker.draw_overlay: one display list per frame instead of one host
round trip per circle.
"""
import numpy as np

LINE_AA = 16        # cv2's value (a cv module handed in need not carry the constant)

_BOX_EDGES = ((0, 1), (1, 2), (2, 3), (3, 0), (0, 4), (1, 5), (2, 6), (3, 7), (4, 5), (5, 6), (6, 7), (7, 4))


def _int_pt(pt):
    return (int(pt[0]), int(pt[1]))


class Draw:
    def __init__(self, logger=None, cv=None):
        if cv is None:
            from . import cv_hip as cv
        self.logger = logger
        self.cv = cv

    def draw_boxes(self, img, imgpts):
        """draw.py:19-60: the twelve edges of a box whose eight projected corners are imgpts"""
        if not np.all(imgpts):
            raise ValueError('Image points are empty.')
        ipoints = [tuple(int(v) for v in pt) for pt in np.round(imgpts).astype(int).reshape(-1, 2)]
        for i, j in _BOX_EDGES:
            self.cv.line(img, ipoints[i], ipoints[j], (0, 255, 0), 1, LINE_AA)

    def draw_2d_pts(self, draw_frame, imgpts):
        """draw.py:63-118: the outline of every tag (four points each, truncated) that lies inside draw_frame whole"""
        imgpts = np.asarray(imgpts)
        max_height, max_width = draw_frame.shape[:2]
        for i in range(0, len(imgpts), 4):
            points = [_int_pt(pt) for pt in imgpts[i:i + 4].reshape(-1, 2)]
            if any(x >= max_width or x < 0 or y >= max_height or y < 0 for x, y in points):
                continue
            for k in range(4):
                self.cv.line(draw_frame, points[k], points[(k + 1) % 4], (255, 255, 255), 5, LINE_AA)

    def draw_squares_and_3d_pts(self, img, draw_frame, imgpts):
        """draw.py:120-153: a red dot on every projected point inside img, then draw_2d_pts.  (The reference tests the dots against
        1280 x 720 whatever the frame; here it is img's own size.)"""
        if not np.all(imgpts):
            raise ValueError('Image points are empty.')
        height, width = img.shape[:2]
        for x, y in np.round(imgpts).astype(int).reshape(-1, 2):
            if 0 <= y < height and 0 <= x < width:
                self.cv.circle(img, (int(x), int(y)), 5, (0, 0, 255), -1)
        self.draw_2d_pts(draw_frame, imgpts)

    def draw_corners(self, img, detection):
        """draw.py:156-189: the detection's box and centre (the tag id text is not drawn)"""
        pts = [_int_pt(pt) for pt in detection.corners]
        for k in range(4):
            self.cv.line(img, pts[k], pts[(k + 1) % 4], (0, 255, 0), 5)
        self.cv.circle(img, _int_pt(detection.center), 5, (0, 255, 255), -1)
