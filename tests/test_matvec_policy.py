"""The plan of the encrypted matrix-vector product (pailliercryptolib_amd/csrc/policy.cpp: matvec_geometry / matvec_slices /
matvec_window) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and run here -- the shapes
tools/bench_matvec.py measures and the edges (one row, one column, fewer columns than slices wanted, one-bit weights).
What it steers: pgpu_batch_ct_matvec, the fused form of a map the reference composes from CipherText::operator*
(ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_matvec_plan_policy(tmp_path):
    exe = str(tmp_path / "matvec_policy_tests")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "matvec_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
