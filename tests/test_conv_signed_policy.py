"""The plans of the signed-weight convolution and sparse product on the CPU.

1. pailliercryptolib_amd/csrc/policy.cpp: conv_signed_plan / spmv_signed_window / spmv_signed_products -- pure host logic,
   compiled with g++ from policy.cpp alone (tests/cpp/conv_signed_policy_tests.cpp) and run here: the unsigned rules with the
   cap held against 2^w + 1 rows per element and 3 (E - 1) products more for the inversion, at the shapes
   tools/bench_conv_signed.py measures and the edges -- a shape at the edge of kMatvecTableCap takes a smaller window or a
   smaller tile than the unsigned plan, the forced knobs clamp.
2. The contract of the host-side plan queries pgpu_ct_conv2d_signed_plan / pgpu_ct_spmv_signed_plan (ctypes; no device): the
   unsigned queries' arguments and fields, table bytes at 2^w + 1 rows per element, products including the inversion, and
   the unsigned queries' refusals."""
import ctypes
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pailliercryptolib_amd", "csrc")
CAP = 256 << 20                                   # policy.hpp: kMatvecTableCap
ROW_BYTES = {1024: 2 * 2 * 19 * 4, 2048: 2 * 4 * 18 * 4, 3072: 2 * 8 * 14 * 4}
KNOBS = ("PGPU_CONV_WINDOW", "PGPU_CONV_TILE", "PGPU_CONV_SLICES", "PGPU_SPMV_WINDOW", "PGPU_SPMV_CHUNK")


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_signed_conv_spmv_plan_policy(tmp_path):
    exe = str(tmp_path / "conv_signed_policy_tests")
    env = {k: v for k, v in os.environ.items() if not k.startswith("PGPU_")}      # the defaults, not a caller's knobs
    subprocess.run(["g++", "-O1", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", "-DPGPU_WITH_4096=0",
                    "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                    os.path.join(ROOT, "tests", "cpp", "conv_signed_policy_tests.cpp"), os.path.join(CSRC, "policy.cpp"), "-o", exe],
                   check=True)
    r = subprocess.run([exe], capture_output=True, text=True, env=env)
    print(r.stdout)
    assert r.returncode == 0, r.stdout[-3000:]
    assert " 0 failed" in r.stdout


# ---- the plan queries ----
def _lib():
    from pailliercryptolib_amd import _capi
    return _capi.lib()


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS:
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def _conv_plan(L, signed, key_bits, shape, e_bits):
    from pailliercryptolib_amd import _capi
    sh = _capi.Conv2dShape(*shape)
    w, s, t, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    fn = L.pgpu_ct_conv2d_signed_plan if signed else L.pgpu_ct_conv2d_plan
    rc = fn(key_bits, ctypes.byref(sh), e_bits, ctypes.byref(w), ctypes.byref(s), ctypes.byref(t), ctypes.byref(tb), ctypes.byref(pr))
    return rc, w.value, s.value, t.value, tb.value, pr.value


def _spmv_plan(L, signed, key_bits, rows, cols, nnz, longest, e_bits):
    w, c, lv, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    fn = L.pgpu_ct_spmv_signed_plan if signed else L.pgpu_ct_spmv_plan
    rc = fn(key_bits, rows, cols, nnz, longest, e_bits, ctypes.byref(w), ctypes.byref(c), ctypes.byref(lv), ctypes.byref(tb), ctypes.byref(pr))
    return rc, w.value, c.value, lv.value, tb.value, pr.value


# (n_img, C_in, H, W, C_out, kh, kw, sh, sw, ph, pw): the bench shapes, two small ones, two at the edge of the cap (2048-bit)
CONV_SHAPES = [(1024, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0), (64, 16, 14, 14, 16, 3, 3, 1, 1, 1, 1), (1, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0),
               (1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0), (5, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1),
               (64, 8, 30, 30, 16, 3, 3, 1, 1, 1, 1), (9, 6, 20, 20, 16, 3, 3, 1, 1, 1, 1)]


@pytest.mark.parametrize("key_bits", [1024, 2048, 3072])
@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv2d_signed_plan_contract(no_knobs, key_bits, shape):
    L = _lib()
    elems, n_img = shape[1] * shape[2] * shape[3], shape[0]
    for e_bits in (1, 32, 70):
        rc, w, s, t, tb, pr = _conv_plan(L, True, key_bits, shape, e_bits)
        urc, uw, us, ut, utb, upr = _conv_plan(L, False, key_bits, shape, e_bits)
        assert rc == urc == 0
        assert 1 <= w <= 6 and 1 <= t <= n_img
        assert tb == t * elems * ((1 << w) + 1) * ROW_BYTES[key_bits] <= CAP
        inv = 3 * (n_img * elems - 1)
        if (w, t) == (uw, ut):                                    # the same plan: the unsigned count plus the inversion
            assert s == us and pr == upr + inv
        else:                                                     # the longer table moved the tile or the window
            assert ut * elems * ((1 << uw) + 1) * ROW_BYTES[key_bits] > CAP and pr >= upr + inv


def test_conv2d_signed_plan_edge_of_the_cap(no_knobs):
    L = _lib()
    _, w, _, t, _, _ = _conv_plan(L, True, 2048, CONV_SHAPES[5], 32)
    _, uw, _, ut, _, _ = _conv_plan(L, False, 2048, CONV_SHAPES[5], 32)
    assert (uw, ut) == (6, 1) and w == 5                          # 7200 elements: 64 rows fit, 65 do not -- a smaller window
    _, w, _, t, _, _ = _conv_plan(L, True, 2048, CONV_SHAPES[6], 32)
    _, uw, _, ut, _, _ = _conv_plan(L, False, 2048, CONV_SHAPES[6], 32)
    assert (uw, ut) == (6, 3) and (w, t) == (6, 2)                # 2400 elements: three images fit, then two -- a smaller tile


def test_conv2d_signed_plan_knobs_and_refusals(no_knobs):
    L = _lib()
    shape = CONV_SHAPES[4]
    no_knobs.setenv("PGPU_CONV_WINDOW", "3")
    no_knobs.setenv("PGPU_CONV_TILE", "2")
    no_knobs.setenv("PGPU_CONV_SLICES", "5")
    rc, w, s, t, tb, pr = _conv_plan(L, True, 2048, shape, 32)
    assert (rc, w, s, t) == (0, 3, 5, 2) and tb == 2 * 42 * 9 * ROW_BYTES[2048]
    assert pr == _conv_plan(L, False, 2048, shape, 32)[5] + 3 * (5 * 42 - 1)
    no_knobs.setenv("PGPU_CONV_WINDOW", "9")
    no_knobs.setenv("PGPU_CONV_TILE", "99")
    no_knobs.setenv("PGPU_CONV_SLICES", "99")
    assert _conv_plan(L, True, 2048, shape, 32)[1:4] == (6, 18, 5)           # clamped to 6, the 18 taps, the 5 images
    for k in KNOBS:
        no_knobs.delenv(k, raising=False)
    from pailliercryptolib_amd import _capi
    sh = _capi.Conv2dShape(*shape)
    assert L.pgpu_ct_conv2d_signed_plan(2048, ctypes.byref(sh), 32, None, None, None, None, None) == 0     # every output is optional
    # what the unsigned query refuses
    assert L.pgpu_ct_conv2d_signed_plan(2048, None, 32, None, None, None, None, None) == -1
    assert L.pgpu_ct_conv2d_signed_plan(0, ctypes.byref(sh), 32, None, None, None, None, None) == -1
    assert L.pgpu_ct_conv2d_signed_plan(2048, ctypes.byref(sh), 0, None, None, None, None, None) == -1
    assert _conv_plan(L, True, 4096, shape, 32)[0] == _conv_plan(L, False, 4096, shape, 32)[0] == -3       # no pair rows
    assert b"pair rows" in L.pgpu_last_error()
    for bad in ((0, 1, 4, 4, 1, 3, 3, 1, 1, 0, 0), (1, 1, 4, 4, 1, 3, 3, 0, 1, 0, 0), (1, 1, 4, 4, 1, 3, 3, 1, 1, 3, 0),
                (1, 1, 4, 4, 1, 5, 3, 1, 1, 0, 0), (1, 1, 1 << 30, 4, 1, 1, 1, 1, 1, 0, 0)):
        assert _conv_plan(L, True, 2048, bad, 32)[0] == _conv_plan(L, False, 2048, bad, 32)[0] == -1, bad


@pytest.mark.parametrize("key_bits", [1024, 2048, 3072])
@pytest.mark.parametrize("rows,cols,nnz,longest,e_bits", [(65536, 65536, 1 << 20, 16, 32), (1024, 1024, 104858, 140, 32),
                                                          (256, 256, 2048, 8, 32), (100, 40, 300, 3, 1), (9, 20, 60, 20, 13),
                                                          (65536, 7200, 1 << 20, 16, 32)])
def test_spmv_signed_plan_contract(no_knobs, key_bits, rows, cols, nnz, longest, e_bits):
    L = _lib()
    rc, w, c, lv, tb, pr = _spmv_plan(L, True, key_bits, rows, cols, nnz, longest, e_bits)
    urc, uw, uc, ulv, utb, upr = _spmv_plan(L, False, key_bits, rows, cols, nnz, longest, e_bits)
    assert rc == urc == 0
    assert (c, lv) == (uc, ulv)                                   # the chunk rule and the fold are carried over
    assert tb == cols * ((1 << w) + 1) * ROW_BYTES[key_bits] and (tb <= CAP or w == 1)
    if w == uw:
        assert pr == upr + 3 * (cols - 1)                         # every column of x is inverted
    else:
        assert w < uw and cols * ((1 << uw) + 1) * ROW_BYTES[key_bits] > CAP and pr >= upr + 3 * (cols - 1)


def test_spmv_signed_plan_edge_knobs_and_refusals(no_knobs):
    L = _lib()
    assert _spmv_plan(L, False, 2048, 65536, 7200, 1 << 20, 16, 32)[1] == 6
    assert _spmv_plan(L, True, 2048, 65536, 7200, 1 << 20, 16, 32)[1] == 5       # 7200 columns: 64 rows fit, 65 do not
    no_knobs.setenv("PGPU_SPMV_WINDOW", "6")
    no_knobs.setenv("PGPU_SPMV_CHUNK", "2")
    assert _spmv_plan(L, True, 3072, 9, 20, 60, 20, 13)[:4] == (0, 6, 2, 5)
    no_knobs.setenv("PGPU_SPMV_WINDOW", "9")
    no_knobs.setenv("PGPU_SPMV_CHUNK", "1")
    assert _spmv_plan(L, True, 3072, 9, 20, 60, 20, 13)[:4] == (0, 6, 1, 6)
    no_knobs.delenv("PGPU_SPMV_WINDOW")
    no_knobs.delenv("PGPU_SPMV_CHUNK")
    assert L.pgpu_ct_spmv_signed_plan(2048, 4, 4, 4, 1, 32, None, None, None, None, None) == 0      # every output is optional
    assert _spmv_plan(L, True, 4096, 64, 64, 64, 1, 32)[0] == -3                  # PGPU_ERR_UNSUPPORTED: no pair rows
    assert b"pair rows" in L.pgpu_last_error()
    for bad in ((0, 4, 4, 4, 1, 32), (2048, 0, 4, 4, 1, 32), (2048, 4, 0, 4, 1, 32), (2048, 4, 4, 0, 1, 32),
                (2048, 4, 4, 4, 0, 32), (2048, 4, 4, 4, 5, 32), (2048, 4, 4, 4, 1, 0), (2048, 2, 4, 7, 3, 32),
                (2048, 1 << 31, 4, 1 << 31, 1, 32), (2048, 4, 4, 1 << 31, 1 << 30, 32)):
        assert _spmv_plan(L, True, *bad)[0] == _spmv_plan(L, False, *bad)[0] == -1, bad


def test_header_and_binding_cover_the_calls():
    from pailliercryptolib_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "pgpu.h")).read()
    for name in ("pgpu_batch_ct_conv2d_signed", "pgpu_batch_ct_spmv_signed", "pgpu_ct_conv2d_signed_plan", "pgpu_ct_spmv_signed_plan"):
        assert "int " + name + "(" in hdr and name in _capi.SYMBOLS
    assert "PGPU_KERNEL_SPMV = 9" in hdr and "PGPU_KERNEL_CONV = 13" in hdr and "PGPU_KERNEL_INVERT = 14" in hdr     # no new kind


def test_no_signed_conv_or_spmv_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = _lib()
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)
    from pailliercryptolib_amd import _capi
    sh = _capi.Conv2dShape(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    assert L.pgpu_batch_ct_conv2d_signed(fake, fake, fake, ctypes.byref(sh), 32, ctypes.byref(out)) == -4 and not out.value
    assert L.pgpu_batch_ct_spmv_signed(fake, fake, fake, fake, fake, 1, 32, ctypes.byref(out)) == -4 and not out.value
