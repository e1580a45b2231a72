"""CPU: the N > 1 path (stream sharding + the single pose gather) with world_size 2 on gloo."""
import os
import socket

import numpy as np
import torch
import torch.multiprocessing as mp

from accurate_aprilgroup_tracking_amd import distributed as D


def _free_port():
    s = socket.socket(); s.bind(("127.0.0.1", 0)); p = s.getsockname()[1]; s.close()
    return p


def _pose_block(streams, frames):
    """deterministic stand-in for tracker output: [frames, streams_local, 8]"""
    out = np.zeros((frames, len(streams), 8))
    for j, sidx in enumerate(streams):
        for f in range(frames):
            out[f, j] = [sidx + 0.1, sidx + 0.2, sidx + 0.3, f * 0.01, f * 0.02, 0.3 + sidx, 1.0, f]
    return out


def _worker(rank, world, port, n_streams, frames, ret):
    os.environ.update(RANK=str(rank), LOCAL_RANK=str(rank), WORLD_SIZE=str(world),
                      MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    r, lr, w = D.init(backend="gloo")
    assert (r, w) == (rank, world)
    mine = D.shard_streams(n_streams, r, w)
    local = torch.from_numpy(_pose_block(list(mine), frames))
    D.barrier()
    allp = D.gather_poses(local)
    assert allp.shape == (world, frames, len(mine), 8)
    for q in range(world):
        ref = _pose_block(list(D.shard_streams(n_streams, q, world)), frames)
        assert np.array_equal(allp[q].numpy(), ref)
    m = D.max_over_ranks(1.0 + rank, torch.device("cpu"))
    assert m == float(world)
    ret[rank] = True
    torch.distributed.destroy_process_group()


def test_shard_streams_partition():
    for n in (1, 7, 8, 64):
        for w in (1, 2, 3, 8):
            parts = [list(D.shard_streams(n, r, w)) for r in range(w)]
            assert sorted(sum(parts, [])) == list(range(n))
            assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1


def test_gather_poses_world2_gloo():
    world, port = 2, _free_port()
    mgr = mp.Manager(); ret = mgr.dict()
    mp.spawn(_worker, args=(world, port, 8, 5, ret), nprocs=world, join=True)
    assert all(ret.get(r) for r in range(world))


def test_single_process_is_passthrough():
    t = torch.arange(24, dtype=torch.float64).reshape(3, 1, 8)
    assert torch.equal(D.gather_poses(t), t.unsqueeze(0))
    assert D.max_over_ranks(2.5, torch.device("cpu")) == 2.5


def _bench_json(cmd, env=None):
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run(cmd, cwd=root, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600, text=True)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [l for l in p.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, p.stdout[-2000:]              # ONE JSON line, from rank 0 only
    return json.loads(lines[0])


def test_bench_self_launch_world2_gloo():
    """`python bench.py --gpus 2` invoked PLAINLY (how the driver calls it) must start its own ranks
    before touching a GPU, run the block timing (barrier / max over ranks) and the pose gather, and relay one JSON line.
    --dry-run swaps the tracker for a stub so this runs on the CPU under gloo."""
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    j = _bench_json([sys.executable, "bench.py", "--gpus", "2", "--steps", "6", "--warmup", "2", "--blocks", "4", "--dry-run"], env)
    assert j["n_gpus"] == 2 and j["steps"] == 6 and j["warmup"] == 2 and j["dry_run"] and j["gather_ok"]
    assert j["gathered_shape"] == [2, 6, 1, 16] and j["timing"]["blocks"] == 4
    assert "dry-run" in j["data"]


def test_bench_self_launch_world8_gloo():
    """BASELINE configs[3] is EIGHT ranks (8 x 1920x1080, one stream per GPU, one gather of the poses per block): the bench's own
    flow -- self-launch, rendezvous, block timing, all_gather, the gather-order check on the real record layout -- with world 8
    on the CPU (VERDICT r4 #7b; the tests of rounds 1-4 stopped at world 2).  Every rank's block must land in its own slot:
    block q holds RANK q's stream (the stub writes the generator's pose of seed 1000 q), and blocks differ from one another."""
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    j = _bench_json([sys.executable, "bench.py", "--gpus", "8", "--workload", "c4", "--steps", "4", "--warmup", "1", "--blocks", "2", "--dry-run"], env)
    assert j["n_gpus"] == 8 and j["steps"] == 4 and j["dry_run"] and j["gather_ok"]
    assert j["gathered_shape"] == [8, 4, 1, 16] and j["config"]["geometry_of"] == "c4"
    # (gather_ok of a dry run IS the gather-order check of the real run at tolerance 1e-12, plus "block q differs from block 0")


def test_bench_under_torchrun_world2_gloo():
    """the driver's N > 1 form: python -m torch.distributed.run ... bench.py --gpus 2 (ranks given by the launcher)"""
    import sys
    env = dict(os.environ, AGT_DIST_BACKEND="gloo")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE"):
        env.pop(k, None)
    j = _bench_json([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
                     "--master-port", str(_free_port()), "bench.py", "--gpus", "2", "--steps", "5", "--warmup", "1", "--blocks", "2", "--dry-run"], env)
    assert j["n_gpus"] == 2 and j["gather_ok"] and j["gathered_shape"] == [2, 5, 1, 16]


def test_bench_plain_run_times_steps_and_dumps_outputs(tmp_path):
    """a plain run times exactly --steps steps (one block), and --dump-outputs writes the records of the last timed step -- the
    same from run to run, since the inputs are (stub tracker on the CPU: the flow of the option, not the kernels)"""
    import sys
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    got = []
    for i in range(2):
        d = tmp_path / ("out%d" % i)
        j = _bench_json([sys.executable, "bench.py", "--gpus", "1", "--steps", "5", "--warmup", "2", "--dry-run", "--dump-outputs", str(d)], env)
        assert j["steps"] == 5 and j["timing"] == {"blocks": 1, "steps_per_block": 5} and j["gathered_shape"] == [1, 5, 1, 16]
        assert sorted(os.listdir(d)) == ["records.npy"]
        got.append(np.load(d / "records.npy"))
    assert got[0].dtype == np.float64 and got[0].shape == (1, 1, 16)
    assert got[0][0, 0, 6] == 1.0 and got[0][0, 0, 8] == 2 + 5          # accepted, the stub's frame counter: warm-up + timed steps
    assert np.array_equal(got[0], got[1])


def test_bench_rejects_world_mismatch():
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    p = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--dry-run", "--steps", "2"], cwd=root, env=env,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, text=True)
    assert p.returncode != 0 and "WORLD_SIZE" in p.stderr
