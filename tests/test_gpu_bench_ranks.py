"""GPU tier: bench.py's N > 1 code path (one process per rank, shard of the BinBundles per rank, two alternating result
buffers, all_gather of the results) rehearsed on the one-GPU box: two ranks on GPU 0, gathered through gloo
(APSU_BENCH_BACKEND=gloo; the driver's multi-GPU runs use the default "nccl" = RCCL, one GPU per rank).  Rank 0 checks that
its own rows arrive unchanged and that every BinBundle's row was filled by some rank."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_two_rank_bench_on_one_gpu():
    env = dict(os.environ, APSU_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--config", "1M-1024-com", "--no-profile", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    line = [l for l in r.stdout.splitlines() if l.startswith("{")][-1]
    d = json.loads(line)
    assert d["n_gpus"] == 2 and d["scaling"] == "strong" and d["value"] > 0
    assert d["gather_check"] == {"rank0_rows_match": True, "all_binbundle_rows_filled": True, "rows": 34}
    assert d["config"]["binbundles_rank0"] == 17
    # the line says who gathered: both ranks, their own step times, the split of the BinBundles
    assert d["distributed"]["world_size"] == 2 and d["distributed"]["backend"] == "gloo"
    assert len(d["distributed"]["ms_local_by_rank"]) == 2 and max(d["distributed"]["ms_local_by_rank"]) == d["ms_per_step"]
    assert d["distributed"]["binbundles_by_rank"] == [17, 17]


def test_two_rank_bench_over_rccl():
    """the driver's launch for N = 2 -- one rank per GPU, the "nccl" (= RCCL) backend, results gathered over xGMI.  Needs two GPUs:
    skipped on the one-GPU boxes this repository is developed on (the N > 1 code path is rehearsed there by the gloo test above and
    by the one-rank RCCL group below; RCCL with more than one rank first runs in the driver's SCALE step)."""
    import torch
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two GPUs")
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("APSU_BENCH_BACKEND", None)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "3", "--warmup", "1",
           "--config", "1M-1024-com", "--no-profile", "--full"]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["n_gpus"] == 2 and d["distributed"]["backend"] == "nccl" and d["distributed"]["world_size"] == 2
    assert d["gather_check"] == {"rank0_rows_match": True, "all_binbundle_rows_filled": True, "rows": 34}
    assert len(d["distributed"]["ms_local_by_rank"]) == 2


def test_rccl_collective_pattern_one_rank():
    """the "nccl" (= RCCL) backend itself, as far as one GPU allows: a one-rank process group running the collective pattern
    of bench.py's N > 1 path (gather ordered after an external stream through events, result buffers alternating)"""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(_free_port()), RANK="0",
               WORLD_SIZE="1")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "rccl_selfcheck.py")], env=env, capture_output=True, text=True,
                       timeout=600, cwd=ROOT)
    assert r.returncode == 0 and "rccl one-rank selfcheck ok" in r.stdout, r.stdout[-2000:] + r.stderr[-4000:]
