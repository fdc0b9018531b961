"""Filtered search on a row-sharded index: world 2 over gloo on cuda:0 (tests/filtered_sharded_worker.py), a filter straddling the
shard boundary at a first row that is not a multiple of 32, d = 768, fp16 and fp8; the merged result against the oracle."""
import json
import os
import socket
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port() -> int:
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_two_ranks_filtered_merge_matches_oracle(native_lib, tmp_path):
    world = 2
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), os.path.join(ROOT, "tests", "filtered_sharded_worker.py"), "--out", str(tmp_path)]
    env = dict(os.environ, PYTHONPATH=ROOT, HSA_ENABLE_IPC_MODE_LEGACY="0")
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=900, env=env, cwd=ROOT)
    assert r.returncode == 0, (r.stdout[-4000:] + "\n" + r.stderr[-6000:])
    for rank in range(world):
        with open(tmp_path / f"rank{rank}.json") as f:
            rec = json.load(f)
        assert rec["world"] == world and rec["checks"] == ["merged_fp16", "merged_fp8"], rec
