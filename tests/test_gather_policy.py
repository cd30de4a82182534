"""The host side of gather / concat / slice of resident batches (pailliercryptolib_amd/csrc/policy.cpp: gather_plan /
gather_descs / gather_slice_descs / gather_image) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and
run here -- once as it is and once under AddressSanitizer + UBSan, as a plain stand-alone program; and
pgpu_batch_gather_plan, the host-side query of the C-ABI, through ctypes on the built library.  What it steers:
pgpu_batch_gather / _concat / _slice, the device-side form of the re-ordering the reference does on host vectors
(CipherText::rotate, ipcl/ciphertext.cpp:96-104; BaseText::getChunk, base_text.cpp)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")
INVALID = -1


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs


def build_policy_binary(tmp_path, name, extra=()):
    exe = str(tmp_path / name)
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC, *extra,
                    os.path.join(ROOT, "tests", "cpp", "gather_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_gather_host_policy(tmp_path):
    exe = build_policy_binary(tmp_path, "gather_policy_tests")
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_gather_host_policy_sanitized(tmp_path):
    """the same program with -fsanitize=address,undefined, run as a plain program (the runtime is linked in)"""
    exe = build_policy_binary(tmp_path, "gather_policy_tests_san",
                              ("-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"))
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout, r.stderr[-3000:])
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-3000:])
    assert " 0 failed" in r.stdout and "ERROR" not in r.stderr and "runtime error" not in r.stderr


@pytest.fixture(scope="module")
def library():
    """the cross-compiled library: the plan query is host code and needs no device"""
    from pailliercryptolib_amd import build
    build.build_pgpu()
    L = ctypes.CDLL(os.path.join(ROOT, "pailliercryptolib_amd", "libpgpu.so"))
    L.pgpu_batch_gather_plan.argtypes = [ctypes.c_size_t, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int),
                                         ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]
    L.pgpu_batch_gather_plan.restype = ctypes.c_int
    return L


def query(L, row_bytes, n_out=1000):
    lanes, rows, vec = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    rc = L.pgpu_batch_gather_plan(row_bytes, n_out, ctypes.byref(lanes), ctypes.byref(rows), ctypes.byref(vec))
    return rc if rc else (lanes.value, rows.value, vec.value)


def test_plan_query_of_the_library(library):
    L = library
    # (lanes per row, rows per wavefront, bytes per access)
    assert query(L, 8) == (1, 64, 8)            # words = 1
    assert query(L, 24) == (4, 16, 8)           # words = 3
    assert query(L, 264) == (16, 4, 8)          # words = 33
    assert query(L, 304) == (16, 4, 16)         # pair rows: 1024-, 2048-, 3072-bit keys
    assert query(L, 576) == (16, 4, 16)
    assert query(L, 896) == (16, 4, 16)
    for row in range(8, 2048 + 8, 8):
        lanes, rows, vec = query(L, row)
        assert vec == (16 if row % 16 == 0 else 8) and lanes * rows == 64 and rows >= 4
        assert lanes == min(16, 1 << max(0, (row // vec - 1).bit_length()))
    assert query(L, 0) == INVALID and query(L, 12) == INVALID and query(L, 576, 0) == INVALID
    assert L.pgpu_batch_gather_plan(576, 10, None, None, None) == 0      # every output pointer may be null
    from pailliercryptolib_amd import _capi
    assert {"pgpu_batch_gather", "pgpu_batch_concat", "pgpu_batch_slice", "pgpu_batch_gather_plan"} <= set(_capi.SYMBOLS)
    assert all(hasattr(L, s) for s in ("pgpu_batch_gather", "pgpu_batch_concat", "pgpu_batch_slice"))
