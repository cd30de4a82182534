"""The host schedule of the encrypted weighted sum of K resident batches (pailliercryptolib_amd/csrc/policy.cpp:
wsum_slices / wsum_wide_pays / wsum_geometry / wsum_plan) on the CPU: pure host logic, compiled with g++ from policy.cpp
alone and run here -- the step lists of ragged weights (every set bit exactly once, the step and product counts of the
formulas, slices that partition the terms), S and the form by the carried-over rules, the forced knobs and the refusals;
and pgpu_ct_weighted_sum_plan, the host-side query of the C-ABI, through ctypes on the built library.  What it steers:
pgpu_batch_ct_weighted_sum, the fused form of a sum the reference composes from CipherText::operator*
(ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72)."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")
INVALID, UNSUPPORTED = -1, -3


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs


def build_policy_binary(tmp_path):
    exe = str(tmp_path / "wsum_policy_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "wsum_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_wsum_schedule_policy(tmp_path):
    exe = build_policy_binary(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout


@pytest.fixture(scope="module")
def library():
    """the cross-compiled library: the plan query is host code and needs no device"""
    from pailliercryptolib_amd import build
    build.build_pgpu()
    L = ctypes.CDLL(os.path.join(ROOT, "pailliercryptolib_amd", "libpgpu.so"))
    L.pgpu_ct_weighted_sum_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.c_size_t, ctypes.c_void_p, ctypes.c_int,
                                            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                            ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t),
                                            ctypes.POINTER(ctypes.c_size_t)]
    L.pgpu_ct_weighted_sum_plan.restype = ctypes.c_int
    return L


def query(L, key_bits, count, weights, n_terms=None, w_words=None):
    """-> rc, or (lanes, limbs, slices, steps, products)"""
    g, k, s, st, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    if weights is None:
        arr, ww, n = None, w_words or 0, n_terms
    else:
        n = len(weights) if n_terms is None else n_terms
        ww = max(1, (max(v.bit_length() for v in weights) + 63) // 64) if w_words is None else w_words
        wn = max(ww, 1)
        arr = (ctypes.c_uint64 * (len(weights) * wn))(*[(v >> (64 * j)) & (2 ** 64 - 1) for v in weights for j in range(wn)])
    rc = L.pgpu_ct_weighted_sum_plan(key_bits, count, n, arr, ww, ctypes.byref(g), ctypes.byref(k), ctypes.byref(s),
                                     ctypes.byref(st), ctypes.byref(pr))
    return rc if rc else (g.value, k.value, s.value, st.value, pr.value)


def test_plan_query_of_the_library(library, monkeypatch):
    for name in ("PGPU_WSUM_SLICES", "PGPU_WSUM_WIDE"):
        monkeypatch.delenv(name, raising=False)
    L = library
    rng = random.Random(1)
    w = [rng.getrandbits(32) | (1 << 31) for _ in range(16)]
    pops = sum(bin(v).count("1") for v in w)
    # 65536 elements fill the chip: one slice, the (4,18) form; 31 squarings and (popcounts - 1) products per element
    assert query(L, 2048, 65536, w) == (4, 18, 1, 31 + pops - 1, 65536 * (31 + pops - 1))
    # 256 elements: 4 slices of 4 terms, each with its own 31 squarings, 3 fold products; 1024 chains: the (8,9) form
    lanes, limbs, slices, steps, products = query(L, 2048, 256, w)
    per_slice = [31 + sum(bin(v).count("1") for v in w[4 * s:4 * s + 4]) - 1 for s in range(4)]
    assert (lanes, limbs, slices, steps, products) == (8, 9, 4, max(per_slice), 256 * (sum(per_slice) + 3))
    # no weights: no squarings; the cap is two terms per slice
    assert query(L, 2048, 65536, None, 16) == (4, 18, 1, 15, 65536 * 15)
    assert query(L, 2048, 256, None, 16) == (8, 9, 8, 1, 256 * 15)
    # zero weights cost nothing; slices of zeros are dropped; all zero: nothing at all
    assert query(L, 1024, 10, [0, 0, 0, 0, 5, 0, 0, 0]) == (2, 19, 1, 3, 10 * 3)
    assert query(L, 3072, 10, [0, 0]) == (8, 14, 1, 0, 0)
    assert query(L, 3072, 10, [1]) == (8, 14, 1, 0, 0)                     # a copy
    # wide weights
    assert query(L, 1024, 1000000, [1 << 99, 1]) == (2, 19, 1, 99 + 1, 1000000 * 100)
    # the knobs are read at every call
    monkeypatch.setenv("PGPU_WSUM_SLICES", "2")
    monkeypatch.setenv("PGPU_WSUM_WIDE", "0")
    assert query(L, 2048, 256, w)[:3] == (4, 18, 2)
    monkeypatch.setenv("PGPU_WSUM_WIDE", "1")
    assert query(L, 2048, 65536, w)[:3] == (8, 9, 2)
    monkeypatch.delenv("PGPU_WSUM_SLICES")
    monkeypatch.delenv("PGPU_WSUM_WIDE")
    # refusals
    assert query(L, 0, 10, w) == INVALID and query(L, 2048, 0, w) == INVALID
    assert query(L, 2048, 10, w, n_terms=0) == INVALID and query(L, 2048, 10, None, 0) == INVALID
    assert query(L, 2048, 10, None, 65536) == INVALID and query(L, 2048, 100000, None, 65535)[2:] == (1, 65534, 100000 * 65534)
    assert query(L, 2048, 10, w, w_words=0) == INVALID and query(L, 2048, 10, w, w_words=-1) == INVALID
    assert query(L, 2048, 10, None, 3, w_words=0) == (8, 9, 1, 2, 20)      # w_words is not read without weights
    assert query(L, 3212, 10, w) == UNSUPPORTED and query(L, 4096, 10, w) == UNSUPPORTED
    assert query(L, 3211, 10, w)[:2] == (8, 14) and query(L, 1065, 10, w)[:2] == (2, 19) and query(L, 1066, 10, w)[:2] == (8, 9)
