"""The plan images of the aggregation calls (pailliercryptolib_amd/csrc/policy.cpp: PlanImage, segsum_image / spmv_image /
segscan_image / wsum_image) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and run here -- section
offsets and total size against the layout written out by hand, every section's bytes against its source vector, and the
partial regions / totals and carries of consecutive levels never sharing a row.  What it steers: the one upload of
pgpu_batch_ct_segment_sum / _spmv / _segment_scan / _weighted_sum (csrc/capi_aggregate.inc), where a wrong offset would
otherwise show only as a wrong ciphertext on the GPU."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


def build_binary(tmp_dir):
    exe = os.path.join(str(tmp_dir), "plan_image_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "plan_image_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_plan_images(tmp_path):
    exe = build_binary(tmp_path)
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
