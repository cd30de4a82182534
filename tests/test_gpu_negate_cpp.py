"""Builds and runs the C++ tests of ipcl::ext::negate / ipcl::ext::subtract (tests/cpp/ipcl_negate_tests.cpp;
include/ipcl/ext/arith.hpp) on the GPU: the batched inversion against host BigNumber arithmetic, through decrypt, against
the exponentiation by n - 1 of the reference's operator (CipherText::operator*, ipcl/ciphertext.cpp:83-107), and on the
results of segmentSum without leaving the device.  The binary is compiled here with g++ (host code only; the kernels are in
libpgpu.so)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "pailliercryptolib_amd")


def build_test_binary():
    exe = os.path.join(CPP, "ipcl_negate_tests.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
                    os.path.join(CPP, "ipcl_negate_tests.cpp"), "-L" + LIBDIR, "-lipcl_amd", "-lpgpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def test_arith_header_compiles_and_links():
    """CPU-side check: the extension header compiles as client code and links against the libraries."""
    from pailliercryptolib_amd import build as b
    b.build_pgpu()
    b.build_ipcl()
    assert os.path.exists(build_test_binary())


@pytest.mark.gpu
def test_negate_cpp_suite_on_gpu():
    from pailliercryptolib_amd import build as b
    b.build_pgpu()
    b.build_ipcl()
    exe = build_test_binary()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, "C++ negate / subtract tests failed"
    assert " 0 failed" in r.stdout
