"""The dense model learned from a recording (include/agt_model.h -> libagt_model.so).

The dense photometric stage (Context.dense_refine, StreamTracker.dense_model) takes samples X_i on the tag planes and a template T_i.
`build_dense_model` makes the template from frames with known poses -- the tracker's accepted records, or the frame poses
`group_calib.calibrate_group` returns: per sample the mean of its bilinear observations over the frames in which its tag is seen at
less than max_view_deg (the tracker's visibility rule) and the sample falls inside the dense stage's validity window; a second,
clipped pass drops the observations that lie far from the first pass's mean (an occluder, a glint).  The accumulation runs on the
device, FP64, in frame order: a result does not depend on how the recording was cut into calls.
"""
import numpy as np

from . import modellib as ML

UPLOAD_CHUNK = 64            # frames per upload of a host (numpy / memory-mapped) recording


def _as_group(extrinsics_or_group):
    """-> {"tags": {"<id>": {"size":, "extrinsics": [tx ty tz rx ry rz]}}} from that, its "tags" object or formats.load_april_group's dict"""
    g = extrinsics_or_group
    if isinstance(g, dict) and set(g) == {"tags"} and isinstance(g["tags"], dict):
        return g
    tags = {}
    for key, v in g.items():
        if isinstance(v, dict):
            tags[str(key)] = {"size": float(v["size"]), "extrinsics": [float(x) for x in v["extrinsics"]]}
        else:
            size, tvec, rvec = v[:3]
            tags[str(key)] = {"size": float(size), "extrinsics": [float(x) for x in np.asarray(tvec).ravel()] + [float(x) for x in np.asarray(rvec).ravel()]}
    return {"tags": tags}


def lattice(extrinsics_or_group, grid=32, extent=0.6):
    """-> (model_xyz f32 (M, 3), sample_tag i32 (M,), tag_corners f32 (T, 4, 3)), M = T * grid * grid: on every tag plane a
    grid x grid lattice over [-extent * size, +extent * size]^2 (the black border and its outer edge included), tags in the order of
    the group -- the order of the tracker's object points."""
    from scipy.spatial.transform import Rotation
    group = _as_group(extrinsics_or_group)
    grid = int(grid)
    if grid < 1:
        raise ValueError("lattice: grid must be at least 1")
    lin = (np.arange(grid) + 0.5) / grid * 2.0 - 1.0
    pts, corners = [], []
    for key in group["tags"]:
        tag = group["tags"][key]
        s = tag["size"] * extent
        uu, vv = np.meshgrid(lin * s, lin * s)
        local = np.stack([uu.ravel(), vv.ravel(), np.zeros(uu.size)], axis=1)
        tvec = np.array(tag["extrinsics"][:3], dtype=np.float32)
        rvec = np.array(tag["extrinsics"][-3:], dtype=np.float32)
        R = Rotation.from_rotvec(rvec.astype(np.float64)).as_matrix()
        pts.append(local @ R.T + tvec.astype(np.float64))
        # the corner model exactly as the tracker gets it (the reference's template order, rotation rounded to f32)
        rad = tag["size"] / 2.0
        init = np.array([[-rad, -rad, 0.0], [-rad, rad, 0.0], [rad, rad, 0.0], [rad, -rad, 0.0]])
        corners.append(init @ R.astype(np.float32).T + tvec.reshape(-1, 3))
    T = len(pts)
    xyz = np.concatenate(pts).astype(np.float32) if T else np.zeros((0, 3), np.float32)
    tag_idx = np.repeat(np.arange(T, dtype=np.int32), grid * grid)
    return xyz, tag_idx, np.asarray(corners).astype(np.float32).reshape(T, 4, 3)


def statistics(n, S, S2):
    """raw sums -> (mean, std), float64; NaN where n = 0.  std = sqrt(max(S2 / n - mean^2, 0))"""
    n = np.asarray(n)
    S, S2 = np.asarray(S, np.float64), np.asarray(S2, np.float64)
    nn = np.where(n > 0, n, 1).astype(np.float64)
    mean = S / nn
    std = np.sqrt(np.maximum(S2 / nn - mean * mean, 0.0))
    return np.where(n > 0, mean, np.nan), np.where(n > 0, std, np.nan)


class DenseModelBuilder:
    """create -> begin_pass -> accumulate ... -> read (-> begin_pass(clip_sigma > 0) -> accumulate ... -> read)"""

    def __init__(self, cameraMatrix, distCoeffs, width, height, tag_corners, model_xyz, sample_tag, max_view_deg=60.0, facing=1, device=None):
        import torch
        if not torch.cuda.is_available():
            raise RuntimeError("accurate_aprilgroup_tracking_amd needs a ROCm GPU (no CPU fallback)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device is None else device)
        self.width, self.height = int(width), int(height)
        with torch.cuda.device(self.device):
            self.handle = ML.DenseModelHandle(cameraMatrix, distCoeffs, width, height, tag_corners, model_xyz, sample_tag, max_view_deg, facing)
        self.M, self.T = self.handle.M, self.handle.T

    def close(self):
        self.handle.close()

    def begin_pass(self, clip_sigma=0.0, sigma_floor=0.0):
        self.handle.begin_pass(clip_sigma, sigma_floor)

    def _device_call(self, frames, poses, use):
        import torch
        assert frames.dtype == torch.uint8 and frames.dim() == 3 and frames.stride(2) == 1, "frames must be u8 [n, H, W] with unit pixel stride"
        assert tuple(frames.shape[1:]) == (self.height, self.width), "frames must be H x W of the model's camera"
        n = frames.shape[0]
        if frames.stride(1) < self.width or (n > 1 and frames.stride(0) < frames.stride(1) * (self.height - 1) + self.width):
            frames = frames.contiguous()                              # (an expanded or overlapping view)
        torch.cuda.current_stream(self.device).synchronize()          # (the library runs on the default stream of the device)
        out = []
        for k in range(0, n, ML.MAX_COUNT):
            m = min(ML.MAX_COUNT, n - k)
            out.append(self.handle.accumulate(frames[k].data_ptr(), frames.stride(1), frames.stride(0), m, poses[k:k + m], None if use is None else use[k:k + m]))
        return np.concatenate(out)

    def accumulate(self, frames, poses, use=None):
        """frames: cuda u8 tensor [n, H, W] with any row stride, or a numpy array (n, H, W) u8 (a memory map too), which is uploaded in
        chunks of at most 64 frames; poses (n, 6) rvec | tvec; use (n,) or None -> frame_obs (n,) i32"""
        import torch
        poses = np.asarray(poses, np.float64).reshape(-1, 6)
        use = None if use is None else np.asarray(use).reshape(-1)
        if poses.shape[0] != len(frames) or (use is not None and use.size != len(frames)):
            raise ValueError("accumulate: %d frames, %d poses%s" % (len(frames), poses.shape[0], "" if use is None else ", %d use bytes" % use.size))
        if isinstance(frames, torch.Tensor):
            if not frames.is_cuda:
                frames = frames.numpy()
            else:
                return self._device_call(frames, poses, use)
        if frames.dtype != np.uint8 or frames.ndim != 3:
            raise ValueError("frames must be u8 (n, H, W)")
        out = [np.zeros(0, np.int32)]
        for k in range(0, frames.shape[0], UPLOAD_CHUNK):
            chunk = torch.from_numpy(np.array(frames[k:k + UPLOAD_CHUNK])).to(self.device)      # (a copy: a memory map may be read-only)
            out.append(self._device_call(chunk, poses[k:k + UPLOAD_CHUNK], None if use is None else use[k:k + UPLOAD_CHUNK]))
        return np.concatenate(out)

    def read(self):
        return self.handle.read()


class DenseModel:
    """model_xyz f32 (M, 3), model_t f32 (M,), sample_tag i32 (M,), n i32, std f64, rejected i32, usable bool (all (M,)),
    frame_obs i32 (F,): observations counted per frame in the last pass, settings: plain numbers"""

    FIELDS = ("model_xyz", "model_t", "sample_tag", "n", "std", "rejected", "usable", "frame_obs")

    def __init__(self, model_xyz, model_t, sample_tag, n, std, rejected, usable, frame_obs, settings=None):
        self.model_xyz = np.ascontiguousarray(np.asarray(model_xyz, np.float32).reshape(-1, 3))
        self.model_t = np.ascontiguousarray(np.asarray(model_t, np.float32).reshape(-1))
        self.sample_tag = np.ascontiguousarray(np.asarray(sample_tag, np.int32).reshape(-1))
        self.n = np.ascontiguousarray(np.asarray(n, np.int32).reshape(-1))
        self.std = np.ascontiguousarray(np.asarray(std, np.float64).reshape(-1))
        self.rejected = np.ascontiguousarray(np.asarray(rejected, np.int32).reshape(-1))
        self.usable = np.ascontiguousarray(np.asarray(usable, bool).reshape(-1))
        self.frame_obs = np.ascontiguousarray(np.asarray(frame_obs, np.int32).reshape(-1))
        self.settings = dict(settings or {})
        M = self.model_xyz.shape[0]
        if not all(a.shape[0] == M for a in (self.model_t, self.sample_tag, self.n, self.std, self.rejected, self.usable)):
            raise ValueError("dense model: arrays of different lengths")

    def compact(self):
        """the usable samples only (what the tracker is given)"""
        k = self.usable
        return DenseModel(self.model_xyz[k], self.model_t[k], self.sample_tag[k], self.n[k], self.std[k], self.rejected[k], self.usable[k],
                          self.frame_obs, self.settings)

    def report(self):
        M, u = self.n.size, int(self.usable.sum())
        obs, rej = int(self.n.sum()), int(self.rejected.sum())
        std = self.std[self.usable]
        lines = ["dense model: %d samples on %d tags, %d usable (%.1f %%)" % (M, np.unique(self.sample_tag).size, u, 100.0 * u / max(M, 1)),
                 "  observations counted %d, rejected by the clip %d (%.1f %%), never seen %d samples" %
                 (obs, rej, 100.0 * rej / max(obs + rej, 1), int((self.n == 0).sum())),
                 "  per sample: observations min %d median %d max %d; std of the usable median %.2f max %.2f gray levels" %
                 (int(self.n.min()) if M else 0, int(np.median(self.n)) if M else 0, int(self.n.max()) if M else 0,
                  float(np.median(std)) if u else 0.0, float(std.max()) if u else 0.0),
                 "  frames %d, with observations %d" % (self.frame_obs.size, int((self.frame_obs > 0).sum()))]
        if self.settings:
            lines.append("  settings: " + ", ".join("%s=%s" % (k, self.settings[k]) for k in sorted(self.settings)))
        return "\n".join(lines)


def build_dense_model(frames, poses, group, cameraMatrix, distCoeffs=None, use=None, grid=32, extent=0.6, max_view_deg=60.0, facing=1,
                      clip_sigma=1.5, sigma_floor=4.0, min_obs=4, max_std=np.inf, fill=128.0, device=None):
    """frames: (F, H, W) u8 -- a cuda tensor or a numpy array / memory map; poses (F, 6) rvec | tvec of the body in each frame;
    use (F,) or None; group: the AprilGroup (april_group.json's dict or formats.load_april_group's).  The plain pass, then one clipped
    pass when clip_sigma > 0.  A sample is usable when it has at least min_obs counted observations and a standard deviation of at
    most max_std; the template of the others is `fill`.  -> DenseModel"""
    xyz, tag, corners = lattice(group, grid, extent)
    H, W = int(frames.shape[1]), int(frames.shape[2])
    b = DenseModelBuilder(cameraMatrix, distCoeffs, W, H, corners, xyz, tag, max_view_deg, facing, device)
    try:
        b.begin_pass()
        frame_obs = b.accumulate(frames, poses, use)
        if clip_sigma > 0:
            b.begin_pass(clip_sigma, sigma_floor)
            frame_obs = b.accumulate(frames, poses, use)
        n, S, S2, rej = b.read()
    finally:
        b.close()
    mean, std = statistics(n, S, S2)
    usable = (n >= max(int(min_obs), 1)) & (std <= max_std)
    model_t = np.where(usable, mean, fill).astype(np.float32)
    settings = dict(grid=int(grid), extent=float(extent), max_view_deg=float(max_view_deg), facing=int(facing), clip_sigma=float(clip_sigma),
                    sigma_floor=float(sigma_floor), min_obs=int(min_obs), max_std=float(max_std), fill=float(fill), width=W, height=H,
                    n_frames=int(frames.shape[0]))
    return DenseModel(xyz, model_t, tag, n, np.where(n > 0, std, 0.0), rej, usable, frame_obs, settings)
