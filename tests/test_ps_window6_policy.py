"""The window rule of the one-lane CRT decrypt (pailliercryptolib_amd/csrc/policy.cpp: pick_decrypt_window, one_lane) on the
CPU: 6 bits for the 1024-bit exponents of the 2048-bit class, by the count of pair squarings and products weighted with their
instruction counts; the other decrypt forms keep their rule; the table cap; a forced width.  Compiled with g++ from policy.cpp
alone.  What it steers: the two exponentiations of PrivateKey::decryptCRT (ipcl/pri_key.cpp:114-146)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_one_lane_window_rule(tmp_path):
    exe = str(tmp_path / "ps_window6_policy_tests")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "ps_window6_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
