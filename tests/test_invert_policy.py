"""The plan of the batched inversion (pailliercryptolib_amd/csrc/policy.cpp: invert_chunk / invert_levels / invert_launches /
invert_products / invert_fits / invert_wide_pays / invert_plan / invert_image; pgpu_ct_negate_plan) on the CPU.  Two parts:
the test program compiled with g++ from policy.cpp alone executes the real plan out of its plan image -- forward passes,
the gather of the totals, one inversion, the walks back -- on small integers modulo a prime: every pass covers every row
exactly once, row t - 1 is read before row t is overwritten, 3 (count - 1) products; and the plan query of the
cross-compiled library (host code, needs no device) is held against a restatement of the rule in Python.  What it steers:
pgpu_batch_ct_negate / pgpu_batch_ct_sub, for which the reference has only the exponentiation by n - 1
(CipherText::operator*, ipcl/ciphertext.cpp:83-107)."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")
SIMDS, WAVES_PER_SIMD, MIN_CHUNK, FORCED_MAX = 256 * 4, 8, 2, 65536      # policy.hpp: kSimds, kSegscanWavesPerSimd, kInvert*
LANES = {1024: 2, 2048: 4, 3072: 8}                                      # G of the pair form per key class


def build_policy_binary(tmp_dir):
    exe = os.path.join(str(tmp_dir), "invert_policy_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "invert_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_invert_plan_policy(tmp_path):
    exe = build_policy_binary(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout


# ---- the rule, restated ----
def model_chunk(bits, count, forced=None):
    if forced is not None and forced >= 2:
        return min(forced, FORCED_MAX)
    chains = WAVES_PER_SIMD * SIMDS * (64 // LANES[bits])
    return min(FORCED_MAX, max(MIN_CHUNK, count // chains))


def model_plan(bits, count, forced=None):
    """the rule applied level by level: (chunk of level 0, levels, launches, products)"""
    levels, m = 1, count
    while m > model_chunk(bits, m, forced):
        m = -(-m // model_chunk(bits, m, forced))
        levels += 1
    return model_chunk(bits, count, forced), levels, 1 if count == 1 else 2 * levels, 3 * (count - 1)


@pytest.fixture(scope="module")
def library():
    """the cross-compiled library: the plan query is host code and needs no device"""
    from pailliercryptolib_amd import build
    build.build_pgpu()
    L = ctypes.CDLL(os.path.join(ROOT, "pailliercryptolib_amd", "libpgpu.so"))
    L.pgpu_ct_negate_plan.argtypes = [ctypes.c_int, ctypes.c_size_t, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                      ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_size_t)]
    L.pgpu_ct_negate_plan.restype = ctypes.c_int
    return L


def query(L, key_bits, count):
    """-> rc, or (chunk, levels, launches, products)"""
    c, lv, la, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    rc = L.pgpu_ct_negate_plan(key_bits, count, ctypes.byref(c), ctypes.byref(lv), ctypes.byref(la), ctypes.byref(pr))
    return rc if rc else (c.value, lv.value, la.value, pr.value)


def test_plan_query_of_the_library(library, monkeypatch):
    for name in ("PGPU_INVERT_CHUNK", "PGPU_INVERT_WIDE"):
        monkeypatch.delenv(name, raising=False)
    L = library
    counts = [1, 2, 3, 7, 8, 9, 64, 65, 300, 2048, 65536, 1 << 20, (1 << 20) + 1, 1 << 24, 1 << 27]
    for bits in LANES:
        for count in counts:
            assert query(L, bits, count) == model_plan(bits, count), (bits, count)
    # written out: a 2048-bit key fills the chip with 131072 chains, so 2^20 elements are chains of 8; the 131072 totals
    # and every level above them are cut into pairs: 17 more levels
    assert query(L, 2048, 1 << 20) == (8, 18, 36, 3 * ((1 << 20) - 1))
    assert query(L, 2048, 1 << 24) == (128, 18, 36, 3 * ((1 << 24) - 1))
    assert query(L, 2048, 64) == (2, 6, 12, 189) and query(L, 2048, 8) == (2, 3, 6, 21) and query(L, 2048, 2) == (2, 1, 2, 3)
    assert query(L, 1024, 1 << 20) == (4, 19, 38, 3 * ((1 << 20) - 1)) and query(L, 3072, 1 << 20) == (16, 17, 34, 3 * ((1 << 20) - 1))
    # count == 1: nothing to multiply forward, one walk back
    assert query(L, 2048, 1) == (2, 1, 1, 0) and query(L, 1024, 1) == (2, 1, 1, 0)
    # the forced chunk (read at every call) and its clamp
    for forced in (2, 3, 8, 100):
        monkeypatch.setenv("PGPU_INVERT_CHUNK", str(forced))
        for bits in LANES:
            for count in counts[:12]:
                assert query(L, bits, count) == model_plan(bits, count, forced), (forced, bits, count)
    monkeypatch.setenv("PGPU_INVERT_CHUNK", "2")
    assert query(L, 2048, 9) == (2, 4, 8, 24) and query(L, 2048, 1) == (2, 1, 1, 0)
    monkeypatch.setenv("PGPU_INVERT_CHUNK", "3")
    assert query(L, 3072, 28) == (3, 4, 8, 81)
    monkeypatch.setenv("PGPU_INVERT_CHUNK", "10000000")
    assert query(L, 2048, 1 << 20) == (FORCED_MAX, 2, 4, 3 * ((1 << 20) - 1))
    monkeypatch.setenv("PGPU_INVERT_CHUNK", "1")                   # below 2: ignored
    assert query(L, 2048, 300) == model_plan(2048, 300)
    # more chains than a descriptor addresses
    monkeypatch.setenv("PGPU_INVERT_CHUNK", "2")
    assert query(L, 2048, 1 << 33) == -1 and query(L, 2048, (1 << 33) - 4)[0] == 2
    monkeypatch.delenv("PGPU_INVERT_CHUNK")
    # no pair rows; zero sizes; null output pointers
    assert query(L, 4096, 10) == -3
    assert query(L, 2048, 0) == -1 and query(L, 0, 10) == -1 and query(L, -5, 10) == -1
    assert L.pgpu_ct_negate_plan(2048, 300, None, None, None, None) == 0
    lv = ctypes.c_int()
    assert L.pgpu_ct_negate_plan(2048, 300, None, ctypes.byref(lv), None, None) == 0 and lv.value == 9
