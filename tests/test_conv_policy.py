"""The plan of the encrypted 2-D convolution (pailliercryptolib_amd/csrc/policy.cpp: conv_plan / conv_products /
conv_slices / conv_geometry) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and run here -- the sizes
of a shape and what a shape alone is refused for, a kernel equal to the image against the matvec's plan, the plan against
the brute-force minimum of the documented product count, the table cap, a short last pass with its own slices, one
oversized image, the forced knobs, and the minibatch the call exists for (1024 images of 1x28x28 under a 2048-bit key,
where the spmv formulation of the same map is held at window 1 by the spmv's own plan functions).
What it steers: pgpu_batch_ct_conv2d."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_conv_plan_policy(tmp_path):
    exe = str(tmp_path / "conv_policy_tests")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "conv_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
