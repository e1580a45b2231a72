"""Scenes of tests/test_gpu_lk_chain_edges.py: short image sequences at small frame sizes, each built to take one of the
frame-chained LK role's rarer paths (agt_lk_chain_body.h), plus the oracle's own LK chain over them.

A scene is a window sliding over the frames of a larger rendered sequence (synthetic.Sequence: twelve moving tags on a static,
band-limited background): the window's offsets are the camera's share of the motion, so background points move too.
kinds:
  slow    the tags' own motion plus a drift of one pixel per frame;
  border  four background corners 26 .. 34 px from an image edge: the 21 x 21 window crosses that edge on level 2 only (+-40 px at
          level 0), and neither the search tile nor the previous-image tile of that level lies inside the image;
  jump    two frames in which everything moves by 14 px (more than the 9 px search margin at level 0 only: followed) and by 40 px
          (10 px at level 2: followed in part, by steps of 15 .. 40 px): the re-stage path inside the iteration loop and the reload of
          the previous-image tile;
  lost    a drift of 5 px per frame carries corners next to the left edge out of the image, each at another frame (sticky status,
          in the middle of a launch group);
  flat    one corner in a constant block (level 0 is rejected by the eigenvalue test: lost at the first frame) and one in a
          pattern that alternates from pixel to pixel along both axes, which the pyramid's 1-4-6-4-1 filter turns into a constant
          (level 1 is rejected while the corner sits on the pattern, and the corner lives on).
"""
import numpy as np

KINDS = ("slow", "border", "jump", "lost", "flat")
STEPS = 11                  # frames tracked after the first: launches of 5 + 5 + 1, 3 + 3 + 3 + 2, ... frames
PAD = 72                    # the rendered frames are larger than the scene by this much on every side


def _offsets(kind):
    """the window's offset inside the rendered frames, per frame (STEPS + 1 of them)"""
    zig = np.array([0, 1, 2, 3, 2, 1, 0, 1, 2, 3, 2, 1])
    if kind == "jump":
        ox = np.array([0, 1, 2, 16, 17, 18, 58, 57, 56, 55, 54, 53])
        oy = np.array([0, 1, 2, 2, 3, 4, 4, 5, 6, 7, 8, 9])
    elif kind == "lost":
        ox = np.array([0, 5, 10, 15, 20, 15, 10, 5, 0, 5, 10, 15])
        oy = zig
    elif kind == "flat":
        ox, oy = 0 * zig, 0 * zig                # (no drift: a pattern of period 2 cannot be followed, only the tags move)
    else:
        ox, oy = zig, zig[::-1]
    return ox + PAD - 10, oy + PAD - 4


class Scene:
    def __init__(self, kind, width, height):
        from accurate_aprilgroup_tracking_amd import synthetic as syn
        assert kind in KINDS
        self.kind, self.width, self.height = kind, width, height
        # (the tags further away than the default 0.30 m: the group's 48 corners fit the small frames)
        seq = syn.Sequence(width + 2 * PAD, height + 2 * PAD, n_tags=12, n_frames=STEPS + 1, seed=31 + KINDS.index(kind), supersample=2,
                           z0=0.42 if width >= 320 else 0.62)
        self.obj, self.K = seq.obj, seq.K
        ox, oy = _offsets(kind)
        big = [seq.frame(k).copy() for k in range(STEPS + 1)]
        c0 = seq.corners(0).copy()
        W, H = width, height
        x0, y0 = int(ox[0]), int(oy[0])
        if kind == "border":
            # (window coordinates -> rendered coordinates: + the first offset)
            c0[0] = (30.3 + x0, H / 2 + 7.6 + y0); c0[5] = (W - 31.4 + x0, H / 2 - 9.2 + y0)
            c0[10] = (W / 2 + 11.7 + x0, 29.5 + y0); c0[15] = (W / 2 - 13.1 + x0, H - 30.8 + y0)
        if kind == "lost":
            for j, x in ((0, 2.4), (5, 7.6), (10, 12.3), (15, 17.8)):
                c0[j] = (x + x0, H / 2 - 30 + 9.0 * j / 5 + y0)
        if kind == "flat":
            bx, by = x0 + 8, y0 + 8                                    # a constant 44 x 44 block, a corner at its centre
            cx, cy = x0 + W - 70, y0 + 6                               # a 64 x 64 alternating pattern, a corner at its centre
            # I = 130 + (-1)^x s(y) + (-1)^y t(x): both gradients live at level 0, and 1 - 4 + 6 - 4 + 1 = 0 along either axis
            rng = np.random.default_rng(5)
            sgn = np.where(np.arange(64) & 1, -1, 1)
            pat = 130 + sgn[None, :] * rng.integers(-50, 51, 64)[:, None] + sgn[:, None] * rng.integers(-50, 51, 64)[None, :]
            for f in big:
                f[by:by + 44, bx:bx + 44] = 131
                f[cy:cy + 64, cx:cx + 64] = pat
            c0[0] = (bx + 22.3, by + 21.6); c0[5] = (cx + 32.4, cy + 31.7)
        self.frames = np.stack([np.ascontiguousarray(big[k][oy[k]:oy[k] + H, ox[k]:ox[k] + W]) for k in range(STEPS + 1)])
        self.c0 = (c0 - np.array([x0, y0])).astype(np.float32)


def oracle_chain(oracle, scene, max_level):
    """the oracle's LK over the scene, status sticky and a lost corner's position carried (as the tracker) ->
    [(points, alive)] per tracked frame"""
    pyr = [oracle.Pyramid(f, 21, max_level) for f in scene.frames]
    pts = scene.c0.copy(); alive = np.ones(len(pts), bool)
    out = []
    for k in range(1, len(scene.frames)):
        nx, status, _ = oracle.calcOpticalFlowPyrLK(pyr[k - 1], pyr[k], pts, winSize=(21, 21), maxLevel=max_level)
        nx = nx.reshape(-1, 2).astype(np.float32); status = status.ravel().astype(bool)
        nx[~alive] = pts[~alive]
        alive = alive & status
        out.append((nx.copy(), alive.copy()))
        pts = nx
    return out
