"""bench.py's command line: a plain run reports the timed steps only, `--full` adds the other measurements and checks, and
`--dump-outputs DIR` writes the result ciphertexts of the last timed step exactly (float64 halves of each 64-bit residue)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

FULL_ONLY = ("throughput_ms_per_query", "roofline", "phases_ms", "one_stream", "ntt_stream", "host_io", "adapter_calls", "wire_io",
             "cpu_baseline", "gather_check")


def _load(d):
    hi, lo = (np.load(os.path.join(d, "result_%s.npy" % k)) for k in ("hi32", "lo32"))
    assert hi.dtype == lo.dtype == np.float64
    return hi.astype(np.uint64) * np.uint64(1 << 32) + lo.astype(np.uint64)


def test_dump_outputs_is_exact_and_bounded(tmp_path, monkeypatch):
    vals = np.random.default_rng(3).integers(0, 2**63, (40, 2, 64), dtype=np.uint64)
    vals[0, 0, :4] = [0, 1, 2**53 + 1, 2**63 - 1]                       # words a plain float64 would round
    table = torch.from_numpy(vals.view(np.int64))
    rows = list(range(39, 3, -1))                                       # BinBundle i sits in row rows[i]
    bench.dump_outputs(str(tmp_path / "all"), table, rows)
    assert (_load(str(tmp_path / "all")) == vals[rows]).all()
    monkeypatch.setattr(bench, "MAX_DUMP_BYTES", len(rows) * 2 * 64 * 16 - 1)
    with pytest.raises(SystemExit, match="limit"):
        bench.dump_outputs(str(tmp_path / "over"), table, rows)
    assert not (tmp_path / "over").exists()


def _bench(out_dir, *extra):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--config", "1M-1024-com",
           "--dump-outputs", out_dir] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_plain_and_full_runs_dump_the_same_checked_results(tmp_path):
    plain = _bench(str(tmp_path / "plain"))
    assert plain["steps"] == 3 and plain["warmup"] == 1 and plain["unit"] == "ms" and plain["higher_is_better"] is False
    assert plain["dtype"] == "u64" and plain["ms_per_step"] == plain["value"] > 0
    assert not [k for k in FULL_ONLY if k in plain]
    full = _bench(str(tmp_path / "full"), "--full", "--no-profile", "--no-host-io")
    assert full["cpu_baseline"]["gpu_result_bit_exact_vs_cpu"] is True      # the timed steps' results, against the CPU oracle
    assert "throughput_ms_per_query" in full
    a, b = _load(str(tmp_path / "plain")), _load(str(tmp_path / "full"))
    assert a.shape == (2 * 17, 2, 4096) and (a == b).all() and a.any()
