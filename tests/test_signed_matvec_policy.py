"""The plans of the signed-weight matvec and matmul (pailliercryptolib_amd/csrc/policy.cpp: matvec_signed_window /
matvec_signed_products / matmul_signed_plan) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and run
here -- window, slices, table bytes (elements * (2^w + 1) * row bytes) and the product count (the unsigned schedule's plus
3 (E - 1) for the inversion) at the shapes tools/bench_matvec_signed.py measures and the edges: one row, one column,
e_bits = 1, and a table that fits the cap only at a smaller window than the unsigned call's."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_signed_plan_policy(tmp_path):
    exe = str(tmp_path / "signed_policy_tests")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "signed_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
