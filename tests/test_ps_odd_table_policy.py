"""The window rule of the one-lane CRT decrypt beside the odd-power window table (pailliercryptolib_amd/csrc/policy.cpp:
ps_one_lane_ops, pick_decrypt_window with one_lane, ps_odd_table) on the CPU: the counts of both table forms, the widths of
the 512-, 1024- and 1536-bit exponents re-weighed with the odd form's counts, the table sizes, and the PGPU_PS_ODD_TABLE
switch.  Compiled with g++ from policy.cpp alone.  What it steers: the two exponentiations of PrivateKey::decryptCRT
(ipcl/pri_key.cpp:114-146)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = str(tmp_path_factory.mktemp("ps_odd") / "ps_odd_table_policy_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "ps_odd_table_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", out],
                   check=True)
    return out


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("switch", [None, "1", "0"])
def test_odd_table_counts_and_window_rule(exe, switch):
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    if switch is not None:
        env["PGPU_PS_ODD_TABLE"] = switch
    r = subprocess.run([exe, "0" if switch == "0" else "1"], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
