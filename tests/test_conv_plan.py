"""The contract of the host-side plan query of the encrypted 2-D convolution, pgpu_ct_conv2d_plan, through ctypes: it needs
no device.  Its products against the documented formula recomputed here, the table cap, the forced knobs, every
PGPU_ERR_INVALID_PARAM of the query, PGPU_ERR_UNSUPPORTED for a 4096-bit key, the spmv formulation's plan of the minibatch
the call exists for -- and, without a device, the call itself fails with PGPU_ERR_NO_DEVICE: there is no CPU fall-back."""
import ctypes
import os

import pytest

from test_conv_model import BIG, SHAPES, out_size, slices_rule
from test_matvec_model import GEOMETRY

KNOBS = ("PGPU_CONV_WINDOW", "PGPU_CONV_TILE", "PGPU_CONV_SLICES")
CAP = 256 << 20
NAMES = ("n_img", "c_in", "h", "w", "c_out", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w")


def _lib():
    from pailliercryptolib_amd import _capi, build
    build.build_pgpu()
    return _capi.lib()


def _plan(key_bits, shape, e_bits):
    from pailliercryptolib_amd import _capi
    L = _lib()
    w, s, t, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    sh = _capi.Conv2dShape(*shape) if shape is not None else None
    rc = L.pgpu_ct_conv2d_plan(key_bits, ctypes.byref(sh) if sh is not None else None, e_bits, ctypes.byref(w), ctypes.byref(s),
                               ctypes.byref(t), ctypes.byref(tb), ctypes.byref(pr))
    return rc, w.value, s.value, t.value, tb.value, pr.value


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS + ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES",
                      "PGPU_SPMV_WINDOW", "PGPU_SPMV_CHUNK"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


def products(g, shape, e_bits, w, tile, slices_of=None):
    """the documented count: per pass over t images t*C_in*H*W*(2^w - 2) + t*n_o*S*e_bits + t*n_o*taps*ceil(e_bits / w) + t*n_o*(S - 1)"""
    n_img, c_in, h, wd, c_out, kh, kw = shape[:7]
    oh, ow = out_size(shape)
    elems, n_o, taps = c_in * h * wd, c_out * oh * ow, c_in * kh * kw

    def one(t):
        S = slices_of(t) if slices_of else slices_rule(g, t * n_o, taps)
        return t * elems * ((1 << w) - 2) + t * n_o * S * e_bits + t * n_o * taps * -(-e_bits // w) + t * n_o * (S - 1)
    return (n_img // tile) * one(tile) + (one(n_img % tile) if n_img % tile else 0)


PLAN_SHAPES = [(2048, s, 32) for s in SHAPES] + [
    (1024, BIG, 13), (3072, BIG, 13),
    (2048, (1, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0), 32), (2048, (64, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0), 32),
    (2048, (1024, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0), 32), (2048, (64, 16, 14, 14, 16, 3, 3, 1, 1, 1, 1), 32),
    (3072, (9, 4, 160, 160, 4, 3, 3, 2, 2, 1, 1), 64), (1024, (3, 1, 1, 1 << 20, 2, 1, 9, 1, 1, 0, 4), 32)]


@pytest.mark.parametrize("key_bits,shape,e_bits", PLAN_SHAPES)
def test_plan_contract(no_knobs, key_bits, shape, e_bits):
    rc, w, s, tile, tb, pr = _plan(key_bits, shape, e_bits)
    assert rc == 0
    g, k = GEOMETRY[key_bits]
    row_bytes = 2 * g * k * 4
    n_img, c_in, h, wd, c_out, kh, kw = shape[:7]
    oh, ow = out_size(shape)
    elems, n_o, taps = c_in * h * wd, c_out * oh * ow, c_in * kh * kw
    assert 1 <= w <= 6 and 1 <= s <= taps and 1 <= tile <= n_img
    assert tb == tile * elems * (1 << w) * row_bytes
    assert tb <= CAP or (tile == 1 and w == 1)               # the cap, but for one oversized image
    assert s == slices_rule(g, tile * n_o, taps)
    assert pr == products(g, shape, e_bits, w, tile)
    # no other window at the tile its table allows (the largest, and a few below it) has fewer products
    for v in range(1, 7):
        t_hi = min(n_img, CAP // (elems * (1 << v) * row_bytes))
        for t in range(t_hi, max(0, t_hi - 8), -1):
            assert products(g, shape, e_bits, v, t) >= pr
    if n_img == 1 and (kh, kw) == (h, wd) and shape[9:] == (0, 0):      # kernel equal to the image: the matvec's plan
        from pailliercryptolib_amd import _capi
        mw, ms, mtb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert _capi.lib().pgpu_ct_matvec_plan(key_bits, c_out, elems, e_bits, ctypes.byref(mw), ctypes.byref(ms), ctypes.byref(mtb)) == 0
        assert (w, s, tile, tb) == (mw.value, ms.value, 1, mtb.value)


def test_minibatch_stays_above_window_1_where_the_spmv_plan_is_at_1(no_knobs):
    """1024 images of 1x28x28, 8 filters of 5x5, 2048-bit key, 32-bit weights: tiled at a wide window; the spmv plan of the
    same map over the same x is held at window 1 by the table over all of x"""
    shape = (1024, 1, 28, 28, 8, 5, 5, 1, 1, 0, 0)
    rc, w, s, tile, tb, pr = _plan(2048, shape, 32)
    assert rc == 0 and w > 1 and tile < 1024 and tb <= CAP
    L = _lib()
    rows, cols, taps = 1024 * 8 * 24 * 24, 1024 * 28 * 28, 25
    sw, sc, sl, stb, spr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    assert L.pgpu_ct_spmv_plan(2048, rows, cols, rows * taps, taps, 32, ctypes.byref(sw), ctypes.byref(sc), ctypes.byref(sl),
                               ctypes.byref(stb), ctypes.byref(spr)) == 0
    assert sw.value == 1 and spr.value > 2 * pr


def test_forced_knobs_are_clamped(no_knobs):
    for k, v in zip(KNOBS, ("4", "2", "5")):
        no_knobs.setenv(k, v)
    elems = 2 * 7 * 3
    rc, w, s, tile, tb, pr = _plan(2048, BIG, 13)
    assert (rc, w, s, tile, tb) == (0, 4, 5, 2, 2 * elems * 16 * 576)
    assert pr == products(4, BIG, 13, 4, 2, lambda t: 5)     # passes of 2, 2 and 1 images, the forced S in each
    for k, v in zip(KNOBS, ("9", "77", "1000")):             # clamped: 1..6, 1..n_img, 1..taps
        no_knobs.setenv(k, v)
    assert _plan(2048, BIG, 13)[:4] == (0, 6, 18, 5)
    for k in KNOBS:
        no_knobs.delenv(k)
    no_knobs.setenv("PGPU_MATMUL_WINDOW", "1")               # another call's knob does not move this plan
    assert _plan(2048, BIG, 13)[1] > 1


def test_refusals(no_knobs):
    L = _lib()
    ok = (2, 3, 5, 4, 2, 3, 2, 1, 1, 1, 0)
    assert _plan(2048, ok, 32)[0] == 0

    def but(**kw):
        return tuple(kw.get(nm, v) for nm, v in zip(NAMES, ok))
    assert _plan(4096, ok, 32)[0] == -3                      # PGPU_ERR_UNSUPPORTED: no pair rows for this key class
    assert b"pair rows" in L.pgpu_last_error()
    bad = [(0, ok, 32), (-5, ok, 32), (2048, ok, 0), (2048, ok, -1), (2048, None, 32)]
    bad += [(2048, but(**{nm: 0}), 32) for nm in NAMES[:9]]                       # any dimension or stride equal to 0
    bad += [(2048, but(pad_h=3), 32), (2048, but(pad_w=2), 32), (2048, but(pad_h=7), 32),      # pad >= kernel
            (2048, but(h=1, kh=4, pad_h=1), 32), (2048, but(w=1, pad_w=0), 32),                # kernel > padded image
            (2048, but(n_img=1 << 40, c_in=1 << 40), 32), (2048, but(c_out=1 << 62), 32),      # a size product beyond size_t
            (2048, but(n_img=1 << 61, c_out=1 << 3), 32), (2048, but(h=1 << 33, w=1 << 33, kh=1, kw=1, pad_h=0), 32),
            (2048, but(n_img=1 << 45, c_in=1, h=1, w=1, kh=1, kw=1, pad_h=0, c_out=1 << 10), (1 << 31) - 1)]      # ... and the product count
    for args in bad:
        assert _plan(*args)[0] == -1, args                   # PGPU_ERR_INVALID_PARAM
    from pailliercryptolib_amd import _capi
    sh = _capi.Conv2dShape(*ok)
    assert L.pgpu_ct_conv2d_plan(2048, ctypes.byref(sh), 32, None, None, None, None, None) == 0      # every output is optional


def test_header_declares_the_call():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pgpu.h")).read()
    assert "int pgpu_batch_ct_conv2d(" in hdr and "int pgpu_ct_conv2d_plan(" in hdr
    assert "typedef struct pgpu_conv2d_shape" in hdr and "PGPU_KERNEL_CONV = 13" in hdr
    assert "size_t n_img, c_in, h, w, c_out, kh, kw, stride_h, stride_w, pad_h, pad_w;" in hdr
    from pailliercryptolib_amd import _capi
    assert [f[0] for f in _capi.Conv2dShape._fields_] == list(NAMES) and ctypes.sizeof(_capi.Conv2dShape) == 11 * ctypes.sizeof(ctypes.c_size_t)


def test_no_conv2d_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from pailliercryptolib_amd import _capi
    L = _lib()
    assert L.pgpu_device_count() == 0
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)                                 # never dereferenced: the readiness check comes first
    sh = _capi.Conv2dShape(1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0)
    rc = L.pgpu_batch_ct_conv2d(fake, fake, fake, ctypes.byref(sh), 32, ctypes.byref(out))
    assert rc == -4 and b"pgpu_init" in L.pgpu_last_error()       # PGPU_ERR_NO_DEVICE
    assert not out.value
