"""Builds and runs the C++ tests of ipcl::ext::gather / concat / slice and of CipherText::rotate on device-resident texts
(tests/cpp/ipcl_index_tests.cpp; include/ipcl/ext/index.hpp) on the GPU: against host vectors after decrypt, rotate on a
resident product against the reference's host rotation (CipherText::rotate, ipcl/ciphertext.cpp:117-133), the chain
rotate -> operator+ -> decrypt, the reference's messages, the host path for texts whose host copy is current.  The binary
is compiled here with g++ (host code only; the kernels are in libpgpu.so)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
LIBDIR = os.path.join(ROOT, "pailliercryptolib_amd")


def build_test_binary():
    exe = os.path.join(CPP, "ipcl_index_tests.bin")
    subprocess.run(["g++", "-O2", "-std=c++17", "-fopenmp", "-I" + os.path.join(ROOT, "include"), "-I" + CPP,
                    os.path.join(CPP, "ipcl_index_tests.cpp"), "-L" + LIBDIR, "-lipcl_amd", "-lpgpu",
                    "-Wl,-rpath," + LIBDIR, "-o", exe], check=True)
    return exe


def test_index_header_compiles_and_links():
    """CPU-side check: the extension header compiles as client code and links against the libraries."""
    from pailliercryptolib_amd import build as b
    b.build_pgpu()
    b.build_ipcl()
    assert os.path.exists(build_test_binary())


@pytest.mark.gpu
def test_index_cpp_suite_on_gpu():
    from pailliercryptolib_amd import build as b
    b.build_pgpu()
    b.build_ipcl()
    exe = build_test_binary()
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(r.stdout[-6000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, "C++ gather / concat / slice / rotate tests failed"
    assert " 0 failed" in r.stdout


@pytest.mark.gpu
def test_rotate_cases_on_oversubscribed_pool():
    """The rotate cases on an in-process pool of two entries (wrapped around the box's one GPU) with a tiny minimum shard:
    pgpu_batch_gather does not shard rows, so CipherText::rotate of a resident text keeps the host path there -- the same
    values, the same messages, no exception from the GPU layer."""
    from pailliercryptolib_amd import build as b
    b.build_pgpu()
    b.build_ipcl()
    exe = build_test_binary()
    env = dict(os.environ, PGPU_POOL_OVERSUBSCRIBE="1", IPCL_GPU_DEVICES="2", PGPU_MIN_SHARD="4", IPCL_EXPECT_POOL="2")
    env.pop("LOCAL_RANK", None)
    env.pop("IPCL_GPU_DEVICE", None)
    r = subprocess.run([exe, "rotate"], capture_output=True, text=True, timeout=600, env=env)
    print(r.stdout[-6000:])
    print(r.stderr[-2000:])
    assert r.returncode == 0, "C++ rotate tests failed on the pool"
    assert "2 tests," in r.stdout and " 0 failed" in r.stdout
