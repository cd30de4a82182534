"""Builds and runs the C++ tests of ipcl::ext::conv2dSigned / conv1dSigned / sparseMatVecSigned
(tests/cpp/ipcl_conv_signed_tests.cpp; include/ipcl/ext/conv.hpp, include/ipcl/ext/linear.hpp) on the GPU: the signed-weight
encrypted convolution and sparse product against decrypt and against the route composed from two unsigned calls and
ipcl::ext::subtract.  The reference's route to a signed weight is CipherText::operator*(PlainText) with w mod n
(ipcl/ciphertext.cpp:83-107).  The binary is compiled here with g++ (host code only; the kernels are in libpgpu.so)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "pailliercryptolib_amd")


def build_test_binary():
    exe = os.path.join(CPP, "ipcl_conv_signed_tests.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
                    os.path.join(CPP, "ipcl_conv_signed_tests.cpp"), "-L" + LIBDIR, "-lipcl_amd", "-lpgpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def test_signed_conv_headers_compile_and_link():
    """CPU-side check: the extension headers compile as client code and link against the libraries."""
    from pailliercryptolib_amd import build as b
    b.build_pgpu()
    b.build_ipcl()
    assert os.path.exists(build_test_binary())


@pytest.mark.gpu
def test_signed_conv_cpp_suite_on_gpu():
    from pailliercryptolib_amd import build as b
    b.build_pgpu()
    b.build_ipcl()
    exe = build_test_binary()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, "C++ signed convolution / sparse product tests failed"
    assert " 0 failed" in r.stdout
