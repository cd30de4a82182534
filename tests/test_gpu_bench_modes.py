"""bench.py's multi-rank mode on the one GPU of a test box: the command line the driver uses for N > 1
(`python -m torch.distributed.run ... bench.py --gpus N`), with one rank over RCCL and with two ranks sharing the device
(gloo; RCCL refuses two ranks on one GPU).  Checks the contract line, not the speed."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _run(nproc, port, extra_env):
    env = dict(os.environ, MASTER_ADDR="127.0.0.1", HSA_ENABLE_IPC_MODE_LEGACY="0", **extra_env)
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={nproc}", "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.join(ROOT, "bench.py"), "--gpus", str(nproc), "--steps", "4", "--warmup", "2",
           "--full"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]           # rank 0 prints ONE JSON line
    assert r.stdout.rstrip("\n").endswith(lines[0]) and len(lines[0].encode()) <= 4096     # last on stdout, compact (bench_line.py)
    line = json.loads(lines[0])
    detail = json.load(open(os.path.join(ROOT, line["detail"])))      # the whole record, written beside the script
    assert detail["value"] == pytest.approx(line["value"], rel=1e-5)
    line["detail_record"] = detail
    return line


def _check(d, n):
    assert d["n_gpus"] == n and d["steps"] == 4 and d["warmup"] == 2 and d["scaling"] == "weak"
    assert d["unit"] == "modexps/s" and d["higher_is_better"] is True and d["value"] > 0
    assert abs(d["value"] - 3 * 8192 * n / (d["ms_per_step"] * 1e-3)) / d["value"] < 1e-3
    assert d["roofline"]["bound"] == "int-alu" and 0 < d["roofline"]["frac"] < 1
    assert d["detail_record"]["config"]["resident_ciphertext_form"].startswith("pair rows")      # the same step as the pool path
    assert d["config"]["secret_table_access"] == "indexed"
    assert d["config"]["batches_in_flight_per_gpu"] == 4                          # (round 5: four lanes, a quarter of the chip each)


def test_one_rank_over_rccl():
    _check(_run(1, 29521, {}), 1)


def test_two_ranks_on_one_device_over_gloo():
    _check(_run(2, 29522, {"BENCH_SINGLE_DEVICE": "1", "BENCH_DIST_BACKEND": "gloo"}), 2)


def test_plain_run_times_k_steps_and_dumps_the_last_one(tmp_path):
    """a plain run (no --full): the headline line over exactly --steps timed steps; --dump-outputs writes the last step's
    ciphertexts and decrypted plaintexts -- the plaintexts are the bench's inputs, spot rows of the ciphertexts the oracle's"""
    import numpy as np
    import bench
    from oracle import paillier_oracle as orc
    from pailliercryptolib_amd.limbs import limbs_to_ints
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
                        "--dump-outputs", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    line = json.loads(r.stdout.rstrip("\n").splitlines()[-1])
    assert line["steps"] == 3 and line["warmup"] == 1 and line["n_gpus"] == 1 and line["unit"] == "modexps/s"
    assert abs(line["value"] - 3 * 8192 / (line["ms_per_step"] * 1e-3)) / line["value"] < 1e-3

    def ints(a):
        return [sum(int(v) << (32 * i) for i, v in enumerate(row)) for row in a]
    m, c = np.load(out / "plaintext.npy"), np.load(out / "ciphertext.npy")
    assert m.dtype == c.dtype == np.float64 and m.shape == (8192, 64) and c.shape == (8192, 128)
    m_host, r_host = bench.synth(0, 8192, 32, 16)
    assert ints(m) == limbs_to_ints(m_host)
    p, q, hs = bench.iso_key()
    opk = orc.PublicKey(p * q, 2048)
    opk.set_djn(hs)
    rows = [0, 4096, 8191]
    assert ints(c[rows]) == opk.encrypt(limbs_to_ints(m_host[rows]), limbs_to_ints(r_host[rows]))
