"""Which pair form does a key get -- from the bit length of n alone (pailliercryptolib_amd/csrc/policy.cpp:
pair_form_for_bits, pub_forms_for_bits) -- swept over every width 16 .. 4200 on the CPU: the form the key builder picks,
the form the matvec / segment_sum / segment_scan / pack plan calls report, the compiled-kernel lists of launch.hpp and the
class table written out in tests/cpp/key_width_policy_tests.cpp must all agree.  Compiled with g++ from policy.cpp alone.
The reference takes any key length that is a multiple of 4 (ipcl/keygen.cpp:101)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
@pytest.mark.parametrize("with_4096", [0, 1])
def test_pair_form_rule_over_every_width(tmp_path, with_4096):
    exe = str(tmp_path / "key_width_policy_tests")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", f"-DPGPU_WITH_4096={with_4096}",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "key_width_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
