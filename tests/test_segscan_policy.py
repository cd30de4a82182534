"""The plan of the encrypted segmented prefix sum (pailliercryptolib_amd/csrc/policy.cpp: segscan_chunk / segscan_levels /
segscan_products / segscan_fits / segscan_plan) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and
run here.  The test program executes the real plan -- the up-sweep SegsumChunks and the scan descriptors, level by level
-- on small integers modulo a prime and compares with the naive prefix and suffix products: ranges inside the batch,
store ranges that are disjoint and cover every row once, carries that an earlier launch wrote, the product and level
counts, the chunk rule and the forced chunk.  What it steers: pgpu_batch_ct_segment_scan, the fused form of a running sum
the reference composes from CipherText::operator+ (ipcl/ciphertext.cpp:35-72) element by element."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


def build_policy_binary(tmp_dir):
    exe = os.path.join(str(tmp_dir), "segscan_policy_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "segscan_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_segscan_plan_policy(tmp_path):
    exe = build_policy_binary(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
