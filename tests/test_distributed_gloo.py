"""CPU, world_size 2, gloo: the sharding + all-gather layer the multi-GPU bench uses (RCCL on the GPU box)."""
import os
import subprocess
import sys

WORKER = r'''
import os, sys
import torch, torch.distributed as dist
sys.path.insert(0, os.environ["NLML_REPO"])
from nlml_hpe_amd.distributed import PoseGatherer, gather_poses, shard_bounds
dist.init_process_group("gloo")
r, w = dist.get_rank(), dist.get_world_size()
for n in (11, 16, 1):
    full = torch.arange(n * 3, dtype=torch.float32).reshape(n, 3)
    s, e, per = shard_bounds(n, w, r)
    got = gather_poses(full[s:e], n)
    assert torch.equal(got, full), (n, got)
g = PoseGatherer(4, w, "cpu")
for i in range(5):                                     # more submissions than ring slots
    g.submit(torch.full((4, 3), float(r * 10 + i)))
last = g.drain()
assert last.shape == (4 * w, 3)
assert all(float(last[4 * k, 0]) == 10 * k + 4 for k in range(w)), last
try:
    g.submit(torch.zeros(3, 3))
    raise SystemExit("shape check missing")
except ValueError:
    pass
dist.barrier()
dist.destroy_process_group()
print("rank", r, "ok")
'''


def test_shard_and_gather_world2(tmp_path, repo_root):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    env = dict(os.environ, NLML_REPO=repo_root, MASTER_ADDR="127.0.0.1")
    port = 29500 + (os.getpid() % 400)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
           "--master-addr", "127.0.0.1", "--master-port", str(port), str(script)]
    res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    assert res.stdout.count("ok") == 2


SPAWN_WORKER = r'''
import os, sys, time
import torch, torch.distributed as dist
mode = sys.argv[1]
r = int(os.environ["RANK"])
assert int(os.environ["LOCAL_RANK"]) == r and os.environ["MASTER_ADDR"] == "127.0.0.1"
if mode == "fail":
    if r == 1:
        sys.exit(3)
    time.sleep(60)              # rank 0 must be stopped by the launcher, not run to the end
    sys.exit(0)
dist.init_process_group("gloo")
t = torch.tensor([float(r + 1)])
dist.all_reduce(t)
if r == 0:
    print('{"n_gpus": %d, "sum": %g}' % (dist.get_world_size(), float(t)), flush=True)
dist.destroy_process_group()
'''


def test_bench_self_launch_spawns_ranks_and_propagates_failure(tmp_path, repo_root):
    """`python bench.py --gpus N` without a launcher (bench.spawn_ranks): N children with the torchrun env contract, rank 0's
    stdout relayed, any failing rank makes the launcher return non-zero and stops the others."""
    script = tmp_path / "spawn_worker.py"
    script.write_text(SPAWN_WORKER)
    drv = ("import sys; sys.path.insert(0, %r); import bench; "
           "sys.exit(bench.spawn_ranks(2, script=%r, argv=[sys.argv[1]]))" % (repo_root, str(script)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    ok = subprocess.run([sys.executable, "-c", drv, "ok"], env=env, capture_output=True, text=True, timeout=300)
    assert ok.returncode == 0, ok.stdout + ok.stderr
    lines = [l for l in ok.stdout.splitlines() if l.startswith("{")]
    assert lines == ['{"n_gpus": 2, "sum": 3}'], ok.stdout
    import time
    t0 = time.time()
    bad = subprocess.run([sys.executable, "-c", drv, "fail"], env=env, capture_output=True, text=True, timeout=300)
    assert bad.returncode == 3, (bad.returncode, bad.stderr)
    assert time.time() - t0 < 45, "the surviving rank was not stopped"


def test_bench_self_launch_deadline_and_profiler_refusal(tmp_path, repo_root):
    """A rank that never finishes (stuck in a collective) is terminated at the launcher's deadline and the launcher returns
    non-zero; under a profiler preload the launcher refuses to start ranks at all (that hop is an exec after GPU init)."""
    script = tmp_path / "hang_worker.py"
    script.write_text("import time\ntime.sleep(120)\n")
    drv = ("import sys; sys.path.insert(0, %r); import bench; "
           "sys.exit(bench.spawn_ranks(2, script=%r, argv=[]))" % (repo_root, str(script)))
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "ROCP_TOOL_LIBRARIES", "LD_PRELOAD")}
    import time
    t0 = time.time()
    res = subprocess.run([sys.executable, "-c", drv], env=dict(env, NLML_BENCH_DEADLINE_S="3"), capture_output=True, text=True, timeout=120)
    assert res.returncode == 124, (res.returncode, res.stderr)
    assert time.time() - t0 < 60
    res = subprocess.run([sys.executable, "-c", drv], env=dict(env, LD_PRELOAD="/nonexistent/librocprofiler-sdk-tool.so"),   # (ld.so ignores a missing preload)
                         capture_output=True, text=True, timeout=120)
    assert res.returncode == 2 and "profiler" in res.stderr, (res.returncode, res.stderr)


def test_bench_dump_outputs_caps_each_array(tmp_path):
    """bench.py --dump-outputs: an array within the cap is written whole; a larger one as the evenly strided sample of its rows
    that fits under the cap (the same rows for the same shape, so two builds' dumps compare row for row)."""
    import numpy as np
    import bench
    small = np.arange(65536 * 3, dtype=np.float32).reshape(65536, 3)
    bench.dump_array(str(tmp_path / "d"), "pose", small)
    assert np.array_equal(np.load(tmp_path / "d" / "pose.npy"), small)
    n = bench.DUMP_MAX_BYTES // 12 * 2 + 5                   # just over twice the cap in rows of three f32
    big = np.arange(n * 3, dtype=np.float32).reshape(n, 3)
    bench.dump_array(str(tmp_path / "d"), "pose_gathered", big)
    got = np.load(tmp_path / "d" / "pose_gathered.npy")
    assert got.nbytes <= bench.DUMP_MAX_BYTES and got.dtype == np.float32
    assert np.array_equal(got, big[::3])                     # the smallest whole stride that fits
