"""The plan of the bucket-method encrypted matvec (pailliercryptolib_amd/csrc/policy.cpp: bucket_plan / bucket_products /
bucket_depth / bucket_sort) on the CPU: pure host logic, compiled with g++ from policy.cpp alone and run here -- the
product and depth bounds against a step-by-step walk of the schedule, the window under the cap, ties, the forced knobs and
their clamping, W == 1 and nb == 1, the shapes the call is meant for, and the digit-aware sort against segsum_sort.  What
it steers: pgpu_batch_ct_matvec_bucket, the fused form of a map the reference composes from CipherText::operator*
(ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")


def clean_env():
    return {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs


def build_policy_binary(tmp_path):
    exe = str(tmp_path / "bucket_policy_tests")
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "bucket_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    return exe


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_bucket_plan_policy(tmp_path):
    exe = build_policy_binary(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, env=clean_env())
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_bucket_bound_against_the_products_the_model_issues(tmp_path):
    """policy.cpp's product bound against the products tests/test_bucket_model.py counts while it runs the schedule on
    weights that fill every bucket (all digits non-zero, every bucket of every window used): the bound may exceed the
    count only by what a chain saves by starting from its first entry instead of a one -- 2^c - 1 products per (row,
    window) in the buckets, 2 per walk, and the U_0 product level 2 never needs"""
    import random
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_bucket_model as model
    exe = build_policy_binary(tmp_path)
    rng = random.Random(20)
    for c, b, e_bits, rows in ((4, 4, 13, 2), (3, 8, 9, 1), (2, 1, 8, 3), (5, 8, 32, 1), (8, 16, 16, 1)):
        W, nb = (e_bits + c - 1) // c, (1 << c) // b
        top = e_bits - c * (W - 1)                                   # bits of the top window
        cols = 3 * (1 << c)
        w = []
        for i in range(rows):
            for j in range(cols):                                    # digit t of column j: 1 + (j + t) mod (2^width - 1): never zero, every bucket hit
                w.append(sum((1 + (j + t) % ((1 << (c if t < W - 1 else top)) - 1)) << (c * t) for t in range(W)))
        x = [rng.randrange(2, model.MOD) for _ in range(cols)]
        cnt = model.Counter()
        got = model.bucket_matvec(x, w, rows, e_bits, c, b, cnt)
        for i in range(rows):
            want = 1
            for j in range(cols):
                want = want * pow(x[j], w[i * cols + j], model.MOD) % model.MOD
            assert got[i] == want
        r = subprocess.run([exe, "count", str(rows), str(cols), str(e_bits), str(c), str(b)], capture_output=True, text=True,
                           env=clean_env(), check=True)
        bound = int(r.stdout.split()[0])
        used = sum((1 << (c if t < W - 1 else top)) - 1 for t in range(W))          # buckets in use per row
        if nb == 1 or b == 1:
            saved_reduce = (nb * 2 * (b - 1) + 2 * (nb - 1) + (b.bit_length() - 1) + nb) - 2 * ((1 << c) - 2)
        else:
            saved_reduce = nb * 1 + 2                                # per block 2 (b - 1) - (2 (b - 2) + 1) = 1; level 2: 2 (nb - 1) - 2 (nb - 2) = 2
        assert bound - cnt.n == rows * used + rows * W * saved_reduce, (c, b, e_bits, bound, cnt.n)
