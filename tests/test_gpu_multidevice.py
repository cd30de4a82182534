"""Tests that turn themselves on when the box has MORE THAN ONE GPU (missing 3): a real pool over every
visible device -- no oversubscription -- must move its key images by RCCL over xGMI, repair nothing, and produce BASELINE
configs[3] (65536 x 3072-bit) and configs[4] (1 M CT+CT / CT x PT) sharded over the GPUs with every element equal to the
C oracle's (SHA-256); the GPUs' decrypt kernels must take the same time within 5 %; and two ranks under
torch.distributed.run broadcast the key over RCCL.  On a 1-GPU box they skip -- except the dry run, which drives the same
worker over an oversubscribed pool of two at reduced sizes so that the worker itself is exercised on every GPU run.
The fan-out these stand in for: /root/reference/module/heqat/heqat/ctrl.c:500-529."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def device_count():
    from pailliercryptolib_amd import _capi
    return _capi.lib().pgpu_device_count()


def run_worker(ndev, count4, count5, timeout=1500, **env):
    e = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", **env)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "multidevice_worker.py"), str(ndev), str(count4), str(count5)],
                       capture_output=True, text=True, timeout=timeout, env=e)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])


def test_worker_dry_run_on_an_oversubscribed_pool(engine):
    """the worker's own logic at reduced sizes, two pool entries on whatever devices there are (1-GPU box: both on it)"""
    res = run_worker(2, 2048, 16384, PGPU_POOL_OVERSUBSCRIBE="1", PGPU_MIN_SHARD="8")
    assert res["pool"] == 2 and res["shards_config4"] == [1024, 1024]
    bad = [k for k, v in res["ok"].items() if not v]
    assert not bad, (bad, res)
    assert res["copies_repaired"] == 0 and res["images_verified"] > 0
    assert set(res["decrypt_kernel_ms"]) == {"0", "1"}


def test_real_pool_configs_4_and_5_every_element(engine):
    n = device_count()
    if n < 2:
        pytest.skip(f"{n} GPU visible: the multi-device run needs at least 2")
    res = run_worker(n, 65536, 1 << 20, timeout=3000)
    assert res["pool"] == n == res["visible"]
    assert res["transport"] == "rccl", res["rccl_note"]          # key images travelled over xGMI by one broadcast
    assert res["copies_repaired"] == 0 and res["images_verified"] >= n
    bad = [k for k, v in res["ok"].items() if not v]
    assert not bad, (bad, res)
    ms = [v for v in res["decrypt_kernel_ms"].values()]
    assert len(ms) == n and max(ms) <= 1.05 * min(ms), res["decrypt_kernel_ms"]   # equal shards, equal GPUs: equal kernel time


def test_two_ranks_broadcast_the_key_over_rccl(engine):
    """bench.py as the driver launches it for N = 2: one process per GPU, backend nccl (= RCCL), the key material broadcast
    from rank 0, every rank's full-size round trip all-reduced into the verdict before rank 0 prints the line"""
    n = device_count()
    if n < 2:
        pytest.skip(f"{n} GPU visible: two ranks over RCCL need two GPUs")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", "29531", os.path.join(ROOT, "bench.py"), "--gpus", "2", "--steps", "4", "--warmup", "2", "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    line = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["value"] > 0 and "nccl" in line["config"]["parallelism"]
