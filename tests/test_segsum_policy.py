"""The plan of the encrypted segmented sum (pailliercryptolib_amd/csrc/policy.cpp: segsum_sort / segsum_chunk /
segsum_levels / segsum_plan) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and run here -- the
stable counting sort, dropped and refused ids, chunks that tile every segment exactly once, the routing of the last level
into the segment's output row, the length order, the level count against the plan query's rule, the forced chunk, empty
and all-NONE input.  What it steers: pgpu_batch_ct_segment_sum, the fused form of a sum the reference composes from
CipherText::operator+ (ipcl/ciphertext.cpp:35-72) after a gather on the host."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


def build_policy_binary(tmp_dir):
    exe = os.path.join(str(tmp_dir), "segsum_policy_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "segsum_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_segsum_plan_policy(tmp_path):
    exe = build_policy_binary(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
