"""The plan of the encrypted sparse matrix-vector product (pailliercryptolib_amd/csrc/policy.cpp: spmv_chunk / spmv_plan /
spmv_window / spmv_products) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and run here -- the chain
descriptors of ragged matrices (every row tiled exactly once, ordered by length, empty rows present, partial rows and fold
levels consistent), the chunk's floor and ceiling, the window under the table cap, the product count, the forced knobs and
the refusals.  What it steers: pgpu_batch_ct_spmv, the fused form of a map the reference composes from
CipherText::operator* (ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs


def build_policy_binary(tmp_path):
    exe = str(tmp_path / "spmv_policy_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "spmv_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_spmv_plan_policy(tmp_path):
    exe = build_policy_binary(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
