"""Scenes of the forward-backward check's tests (test_fb_check.py, test_gpu_fb_check.py): seeded, procedural.

A `synthetic.Sequence` of 12 tags (48 corners); from frame OCC_FROM on an occluder covers tag 0: the tag's bounding box in that
frame plus OCC_PAD px is painted with a fixed texture -- numpy seed 1 noise through a Gaussian of sigma 2, contrast-stretched x 6
about 128 -- that does not move with the tag.  LK follows the tag's corners onto that texture with status 1 and errors of pixels;
tracked back they do not come home.  The oracle compositions below are the expected values of every test: two
`oracle.calcOpticalFlowPyrLK` calls and the float32 rule of include/agt_hip.h (agt_lk_track_fb).
"""
import numpy as np

OCC_FROM = 2          # first occluded frame
OCC_PAD = 14          # px around tag 0's bounding box
OCC_TAG = 0
N_FRAMES = 6
WIN, MAX_LEVEL, FB_PX = 21, 2, 1.0
# (width, height, seed): the two occluder scenes
SCENE_720P = (1280, 720, 1)
SCENE_480P = (640, 480, 0)


def occluder_texture(width, height):
    from scipy.ndimage import gaussian_filter
    noise = np.random.default_rng(1).uniform(0.0, 255.0, (height, width))
    return np.clip((gaussian_filter(noise, 2.0) - 128.0) * 6.0 + 128.0, 0, 255).astype(np.uint8)


class OccludedSequence:
    """frames / corners / truth of a synthetic.Sequence with the occluder painted in from frame OCC_FROM on
    (occluded=False: the clean sequence behind the same interface)"""

    def __init__(self, width, height, seed, n_frames=N_FRAMES, occluded=True, speed=1.0, group_seed=None):
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        self.seq = syn.Sequence(width, height, n_tags=12, n_frames=n_frames, seed=seed, speed=speed, group_seed=group_seed)
        self.width, self.height, self.occluded = width, height, occluded
        self.obj, self.K, self.dist, self.group = self.seq.obj, self.seq.K, self.seq.dist, self.seq.group
        self.rvecs, self.tvecs = self.seq.rvecs, self.seq.tvecs
        self._tex = None
        self._frames = {}

    def __len__(self):
        return len(self.seq)

    def corners(self, k):
        return self.seq.corners(k)

    def box(self, k):
        """the occluder's rectangle in frame k: x0, y0, x1, y1 (exclusive), clipped to the image"""
        c = self.seq.corners(k)[4 * OCC_TAG:4 * OCC_TAG + 4]
        x0, y0 = np.floor(c.min(axis=0)).astype(int) - OCC_PAD
        x1, y1 = np.ceil(c.max(axis=0)).astype(int) + OCC_PAD + 1
        return max(x0, 0), max(y0, 0), min(x1, self.width), min(y1, self.height)

    def frame(self, k):
        if k not in self._frames:
            f = self.seq.frame(k)
            if self.occluded and k >= OCC_FROM:
                if self._tex is None:
                    self._tex = occluder_texture(self.width, self.height)
                x0, y0, x1, y1 = self.box(k)
                f = f.copy()
                f[y0:y1, x0:x1] = self._tex[y0:y1, x0:x1]
            self._frames[k] = f
        return self._frames[k]

    def frames(self):
        return np.stack([self.frame(k) for k in range(len(self))])

    def truth(self, k):
        return np.concatenate([self.rvecs[k].ravel(), self.tvecs[k].ravel()]).astype(np.float64)


def fb_rule(p, back, st_f, st_b, fb_px):
    """the verdict of include/agt_hip.h: float32 max norm, NaN fails -> (status u8, dist f32 with -1 where a pass lost the corner)"""
    p = np.asarray(p, np.float32).reshape(-1, 2); back = np.asarray(back, np.float32).reshape(-1, 2)
    both = (np.asarray(st_f).ravel() != 0) & (np.asarray(st_b).ravel() != 0)
    with np.errstate(invalid="ignore"):
        d = np.maximum(np.abs(p[:, 0] - back[:, 0]), np.abs(p[:, 1] - back[:, 1])).astype(np.float32)
        keep = both & (d < np.float32(fb_px))
    return keep.astype(np.uint8), np.where(both, d, np.float32(-1.0)).astype(np.float32)


def oracle_fb(oracle, prev, nxt, pts, fb_px=FB_PX, win=(WIN, WIN), max_level=MAX_LEVEL, criteria=(3, 30, 0.01), flags=0,
              min_eig=1e-4, next_pts=None, alive=None):
    """The oracle composition -> (next_pts [n,2] f32, status [n] u8, err [n] f32, fb_dist [n] f32, forward status [n] u8).
    prev / nxt: images or oracle.Pyramid objects.  alive (bool [n], tracker mode): a corner that is not alive is not tracked at
    all -- forward status 0, position carried."""
    pts = np.ascontiguousarray(np.asarray(pts, np.float32).reshape(-1, 2))
    nx, st_f, er = oracle.calcOpticalFlowPyrLK(prev, nxt, pts, next_pts, winSize=win, maxLevel=max_level, criteria=criteria,
                                               flags=flags, minEigThreshold=min_eig)
    nx = nx.reshape(-1, 2).copy(); st_f = st_f.ravel().copy(); er = er.ravel().copy()
    if alive is not None:
        nx[~alive] = pts[~alive]; st_f[~alive] = 0; er[~alive] = 0
    back, st_b, _ = oracle.calcOpticalFlowPyrLK(nxt, prev, nx, None, winSize=win, maxLevel=max_level, criteria=criteria,
                                                flags=flags & ~oracle.OPTFLOW_USE_INITIAL_FLOW, minEigThreshold=min_eig)
    st, dist = fb_rule(pts, back, st_f, st_b, fb_px)
    return nx, st, er, dist, st_f
