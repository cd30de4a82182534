"""The encrypted 2-D convolution on resident ciphertexts (pgpu_batch_ct_conv2d; csrc/hensel_conv.hpp) on the GPU:
    out[n][co][oy][ox] = prod_{ci,ky,kx} x[n][ci][oy*sh + ky - ph][ox*sw + kx - pw]^w[co][ci][ky][kx] mod n^2
(a tap outside the image left out), held bit-identical to Python's pow for the 1024-, 2048- and 3072-bit key classes
(32 / 16 / 8 groups per wavefront).  The shapes are those of tests/test_conv_model.py, the smallest at which the mapping
can still go wrong; the 240-output one under forced windows, slices (5 does not divide the 18 taps) and tiles (2: a short
last pass).  Every reference is computed once per shape.  Further: the pgpu_batch_ct_spmv formulation of the same map on
the same resident x, the matvec and the transposed matmul a convolution degenerates to on the same handles, edge weights,
inputs in every form, two layers chained through CRT decrypt against torch.nn.functional.conv2d on int64 tensors, a call
whose short last pass runs on more slices than its full passes, two lanes at once, the refusals, the timing record, a key width off the classes and the Python layer."""
import ctypes
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from test_conv_model import BIG, SHAPES, out_size
from test_gpu_matvec import Case
from test_gpu_pair_rows import Res, key_case  # noqa: F401 -- (Res: the child processes below name it too)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [1024, 2048, 3072]
KNOBS = ("PGPU_CONV_WINDOW", "PGPU_CONV_TILE", "PGPU_CONV_SLICES")
KIND_CONV = 13
POOLING = SHAPES[3]


@pytest.fixture
def knobs(monkeypatch):
    for name in KNOBS + ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_SPMV_WINDOW", "PGPU_SPMV_CHUNK", "PGPU_MATMUL_WINDOW",
                         "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES"):
        monkeypatch.delenv(name, raising=False)

    def force(w=None, t=None, s=None):
        for name, v in zip(KNOBS, (w, t, s)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


def cshape(shape):
    from pailliercryptolib_amd import _capi
    return _capi.Conv2dShape(*shape)


def conv(c, x, wb, shape, e_bits):
    return c.R.op(c.L.pgpu_batch_ct_conv2d, c.pk._h, x, wb, ctypes.byref(cshape(shape)), e_bits)


def live_taps(shape):
    """per output, in output order: [(element of x, index into w)] of the taps inside the image"""
    n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw = shape
    oh, ow = out_size(shape)
    rows = []
    for n in range(n_img):
        for co in range(c_out):
            for oy in range(oh):
                for ox in range(ow):
                    row = []
                    for ci in range(c_in):
                        for ky in range(kh):
                            for kx in range(kw):
                                iy, ix = oy * sh + ky - ph, ox * sw + kx - pw
                                if 0 <= iy < h and 0 <= ix < w:
                                    row.append((((n * c_in + ci) * h + iy) * w + ix, ((co * c_in + ci) * kh + ky) * kw + kx))
                    rows.append(row)
    return rows


def expect(xs, wt, nsq, shape):
    """the definition, with pow"""
    out = []
    for row in live_taps(shape):
        acc = 1
        for e, k in row:
            if wt[k]:
                acc = acc * pow(xs[e], wt[k], nsq) % nsq
        out.append(acc)
    return out


def sizes(shape):
    n_img, c_in, h, w, c_out, kh, kw = shape[:7]
    oh, ow = out_size(shape)
    return n_img * c_in * h * w, c_out * c_in * kh * kw, n_img * c_out * oh * ow


def e_bits_of(shape):
    n_x, n_w, n_out = sizes(shape)
    return 1 if shape == POOLING else 32 if n_out * shape[1] * shape[5] * shape[6] < 1000 else 13


def rand_filter(rng, shape, e_bits):
    n_w = sizes(shape)[1]
    return [1] * n_w if shape == POOLING else [rng.getrandbits(e_bits) for _ in range(n_w)]


def spmv_formulation(c, x, wt, shape, e_bits):
    """CSR rows of the live taps of every output, column numbers into x, the weights replicated"""
    rows = live_taps(shape)
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    ci = np.array([e for r in rows for e, _ in r], dtype=np.uint32)
    wb = c.R.up([wt[k] for r in rows for _, k in r], (e_bits + 63) // 64)
    return c.R.op(c.L.pgpu_batch_ct_spmv, c.pk._h, x, rp.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p), wb,
                  len(rows), e_bits)


@pytest.mark.parametrize("bits", BITS)
def test_conv2d_is_exact_at_every_shape(engine, knobs, bits):
    """x from a resident DJN encrypt and as uploaded plain ciphertext words; the plan the policy picks; x unchanged; the
    spmv formulation on the same resident x; the matvec and the transposed matmul on the same handles"""
    c = Case(engine, bits)
    L, R = c.L, c.R
    rng = random.Random(bits)
    try:
        for shape in SHAPES:
            n_x, n_w, n_out = sizes(shape)
            e_bits = e_bits_of(shape)
            x = c.encrypt([rng.randrange(c.n) for _ in range(n_x)], rng)
            xs = R.down(x)
            wt = rand_filter(rng, shape, e_bits)
            wb = R.up(wt, (e_bits + 63) // 64)
            want = expect(xs, wt, c.nsq, shape)
            y = conv(c, x, wb, shape, e_bits)
            assert L.pgpu_batch_count(y) == n_out and L.pgpu_batch_row_limbs(y) > 0 and L.pgpu_batch_lane(y) == L.pgpu_batch_lane(x)
            assert R.down(y) == want, shape
            assert R.down(x) == xs, shape                                           # x is left unchanged
            assert R.down(conv(c, R.up(xs, 2 * c.nw), wb, shape, e_bits)) == want, shape      # plain ciphertext words
            assert R.down(spmv_formulation(c, x, wt, shape, e_bits)) == want, shape
            n_img, c_in, h, w, c_out, kh, kw = shape[:7]
            if shape == POOLING:                                                    # every output the product of its block
                assert want[0] == xs[0] * xs[1] * xs[6] * xs[7] % c.nsq
            if (kh, kw) == (h, w) and n_img == 1 and shape[9:] == (0, 0):           # kernel equal to the image: the matvec
                assert R.down(R.op(L.pgpu_batch_ct_matvec, c.pk._h, x, wb, c_out, e_bits)) == want
            if (kh, kw) == (1, 1) and n_img == 1:                                   # 1x1 kernel: x is [cols = C_in][n_vec = H*W]
                assert R.down(R.op(L.pgpu_batch_ct_matmul, c.pk._h, x, wb, h * w, c_out, e_bits, 1)) == want
            R.close()
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_forced_windows_slices_and_tiles(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    n_x, n_w, n_out = sizes(BIG)
    e_bits = 13
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(n_x)], rng)
        xs = c.R.down(x)
        wt = rand_filter(rng, BIG, e_bits)
        wb = c.R.up(wt, 1)
        want = expect(xs, wt, c.nsq, BIG)
        assert n_out == 240
        for w in (1, 4, 6):
            for s in (1, 2, 5, 18):                       # 5 does not divide the 18 taps
                for t in (1, 2, 5):                       # 2: passes of 2, 2 and 1 images
                    knobs(w, t, s)
                    assert c.R.down(conv(c, x, wb, BIG, e_bits)) == want, (w, s, t)
                c.R.close()
                x = c.R.up(xs, 2 * c.nw)
                wb = c.R.up(wt, 1)
        knobs()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_weight_edge_cases(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    shape = (1, 2, 4, 3, 5, 2, 2, 1, 1, 1, 1)             # 5 filters of 8 taps, padded on both axes
    n_x, n_w, n_out = sizes(shape)
    taps = 8
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(n_x)], rng)
        xs = c.R.down(x)
        oh, ow = out_size(shape)
        for e_bits in (1, 32, 64, 127):
            top = (1 << e_bits) - 1
            wt = ([0] * taps +                                                    # an all-zero filter: the ciphertext 1
                  [1] * taps +
                  [top] * taps +                                                  # all taps 2^e_bits - 1
                  [rng.getrandbits(e_bits) if j % 3 else 0 for j in range(taps)] +    # zeros scattered
                  [rng.getrandbits(e_bits) for _ in range(taps)])
            want = expect(xs, wt, c.nsq, shape)
            assert all(want[k] == 1 for k in range(oh * ow))
            assert c.R.down(conv(c, x, c.R.up(wt, (e_bits + 63) // 64), shape, e_bits)) == want, e_bits
        # bits at and above e_bits are ignored
        wt = [rng.getrandbits(64) for _ in range(n_w)]
        assert c.R.down(conv(c, x, c.R.up(wt, 1), shape, 13)) == expect(xs, [v & 0x1FFF for v in wt], c.nsq, shape)
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_two_chained_layers_then_decrypt(engine, knobs, bits):
    """the second layer takes the first one's result as it is; Dec mod n against torch's conv2d on int64 CPU tensors:
    plaintexts below 2^20, weights below 2^13, 18 and 12 taps -- the exact sums stay below 2^20 * 2^13 * 18 * 2^13 * 12 < 2^54"""
    import torch
    import torch.nn.functional as F
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    s1 = (2, 2, 6, 5, 3, 3, 3, 1, 1, 1, 1)                # -> [2][3][6][5]
    s2 = (2, 3, 6, 5, 2, 2, 2, 2, 2, 0, 1)                # -> [2][2][3][3]
    try:
        m = [rng.randrange(1 << 20) for _ in range(sizes(s1)[0])]
        w1 = [rng.randrange(1 << 13) for _ in range(sizes(s1)[1])]
        w2 = [rng.randrange(1 << 13) for _ in range(sizes(s2)[1])]
        assert s1[1] * s1[5] * s1[6] <= 100 and s2[1] * s2[5] * s2[6] <= 100
        tm = torch.tensor(m, dtype=torch.int64).reshape(2, 2, 6, 5)
        t1 = F.conv2d(tm, torch.tensor(w1, dtype=torch.int64).reshape(3, 2, 3, 3), stride=(1, 1), padding=(1, 1))
        t2 = F.conv2d(t1, torch.tensor(w2, dtype=torch.int64).reshape(2, 3, 2, 2), stride=(2, 2), padding=(0, 1))
        bound = ((1 << 20) - 1) * ((1 << 13) - 1) * 18 * ((1 << 13) - 1) * 12
        assert bound < 1 << 63 and int(t2.max()) <= bound and int(t2.min()) >= 0      # no int64 wrap in the oracle
        assert sizes(s1)[2] == sizes(s2)[0] and tuple(t2.shape) == (2, 2) + out_size(s2)
        x = c.encrypt(m, rng)
        xs = R.down(x)
        y = conv(c, x, R.up(w1, 1), s1, 13)
        ys = expect(xs, w1, c.nsq, s1)
        assert R.down(y) == ys
        z = conv(c, y, R.up(w2, 1), s2, 13)               # the first layer's result as it is
        assert R.down(z) == expect(ys, w2, c.nsq, s2)
        d = R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, z))
        assert d == [int(v) % c.n for v in t2.flatten().tolist()]
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, y)) == [int(v) % c.n for v in t1.flatten().tolist()]
    finally:
        R.close()


def test_last_pass_on_more_slices_than_a_full_pass(engine, knobs):
    """3072 bits, 9 images of 11 x 11 under 8 filters of 4 x 4 -> 512 outputs per image over 16 taps, in tiles of 8, no
    forced slices: a full pass has 4096 outputs = 512 wavefronts, fill 2 under the cap 16 / 4; the last pass of one image
    64 wavefronts, fill 16: four slices, inside a partial block sized by the larger count.  The query of the call itself
    reports the full passes' count; the two are read off queries with 8 images and with one.  Weights of 2 bits"""
    bits, e_bits, tile = 3072, 2, 8
    c = Case(engine, bits)
    rng = random.Random(bits + 5)
    shape = (9, 1, 11, 11, 8, 4, 4, 1, 1, 0, 0)
    n_x, n_w, n_out = sizes(shape)
    assert (n_out, n_w) == (9 * 512, 8 * 16)
    ps, pt = ctypes.c_int(), ctypes.c_size_t()

    def plan(n_img):
        sh = cshape((n_img,) + shape[1:])
        assert c.L.pgpu_ct_conv2d_plan(bits, ctypes.byref(sh), e_bits, None, ctypes.byref(ps), ctypes.byref(pt), None, None) == 0
        return ps.value, pt.value
    try:
        knobs(None, tile, None)
        full, one, whole = plan(tile), plan(1), plan(9)
        print(f"conv2d plan, {bits} bits, tile {tile}: slices {full[0]} with {tile} images, {one[0]} with one, {whole[0]} with 9")
        assert full == (2, tile) and one == (4, 1) and whole == (2, tile)
        xs = [rng.randrange(1, c.nsq) for _ in range(n_x)]
        wt = rand_filter(rng, shape, e_bits)
        tab = [[pow(x, e, c.nsq) for e in range(4)] for x in xs]         # the weights are below 4: pow once per (x, weight)
        want = []
        for row in live_taps(shape):
            acc = 1
            for e, k in row:
                if wt[k]:
                    acc = acc * tab[e][wt[k]] % c.nsq
            want.append(acc)
        assert c.R.down(conv(c, c.R.up(xs, 2 * c.nw), c.R.up(wt, 1), shape, e_bits)) == want
    finally:
        c.R.close()


def test_two_lanes_at_once(engine, knobs):
    """two threads on different batch lanes, each with its own x and its own shape, the filters uploaded by the main thread
    on its lane; tiles of 2 images over 3 tap slices; three calls in a row per thread, so that the blocks of one lane come
    and go while the other's kernels run"""
    c = Case(engine, 2048)
    L = c.L
    rng = random.Random(12)
    results, errors = {}, []
    shapes = {1: BIG, 2: SHAPES[2]}
    wts = {lane: rand_filter(rng, sh, 13) for lane, sh in shapes.items()}
    xss = {lane: [rng.randrange(1, c.nsq) for _ in range(sizes(sh)[0])] for lane, sh in shapes.items()}
    knobs(None, 2, 3)

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            x = R.up(xss[lane], 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for it in range(3):
                y = R.op(L.pgpu_batch_ct_conv2d, c.pk._h, x, ws[lane], ctypes.byref(cshape(shapes[lane])), 13)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = R.down(y)
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    try:
        ws = {lane: c.R.up(wts[lane], 1) for lane in shapes}         # lane of the main thread: ordered in by events
        ts = [threading.Thread(target=worker, args=(lane,)) for lane in (1, 2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert len(results) == 6
        for lane, sh in shapes.items():
            want = expect(xss[lane], wts[lane], c.nsq, sh)
            for it in range(3):
                assert results[(lane, it)] == want, (lane, it)
    finally:
        c.R.close()


def test_refusals_are_host_side(engine, knobs):
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(9)
    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    ok = (1, 2, 3, 4, 2, 2, 3, 1, 1, 1, 1)                # 24 ciphertexts, 24 taps in all
    try:
        xs = [rng.randrange(1, c.nsq) for _ in range(24)]
        x = R.up(xs, 2 * c.nw)
        xp = c.encrypt(list(range(1, 25)), rng)
        wt = [rng.getrandbits(32) for _ in range(24)]
        wb = R.up(wt, 1)
        other = engine.PublicKey(int(json.load(open(os.path.join(ROOT, "tests", "golden", "aggregate_refusals.json")))["other_n"]["2048"], 16), 2048)
        pair_other = R.op(L.pgpu_batch_ct_add, other._h, R.up(xs, 2 * c.nw), R.up(xs, 2 * c.nw))
        L.pgpu_debug_set_hensel(0)
        try:
            mont_other = R.op(L.pgpu_batch_ct_add, other._h, R.up(xs, 2 * c.nw), R.up(xs, 2 * c.nw))
        finally:
            L.pgpu_debug_set_hensel(1)
        assert L.pgpu_batch_row_limbs(pair_other) > 0 and L.pgpu_batch_is_montgomery(mont_other) == 1
        wide = R.up(xs, 2 * c.nw + 1)
        out = ctypes.c_void_p()
        k = c.pk._h

        def call(key, xb, wbatch, shape, e_bits):
            return L.pgpu_batch_ct_conv2d(key, xb, wbatch, ctypes.byref(cshape(shape)) if shape else None, e_bits, ctypes.byref(out))

        def but(**kw):
            names = ("n_img", "c_in", "h", "w", "c_out", "kh", "kw", "stride_h", "stride_w", "pad_h", "pad_w")
            return tuple(kw.get(nm, v) for nm, v in zip(names, ok))
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)         # drop what the set-up left
            invalid = [((None, x, wb, ok, 32), b"null"), ((k, None, wb, ok, 32), b"null"), ((k, x, None, ok, 32), b"null"),
                       ((k, x, wb, None, 32), b"null")]
            invalid += [((k, x, wb, but(**{nm: 0}), 32), b"must be positive")
                        for nm in ("n_img", "c_in", "h", "w", "c_out", "kh", "kw", "stride_h", "stride_w")]
            invalid += [
                ((k, x, wb, but(pad_h=2), 32), b"pad_h < kh"), ((k, x, wb, but(pad_w=3), 32), b"pad_w < kw"),
                ((k, x, wb, but(h=1, c_in=6, kh=4, pad_h=1), 32), b"kh <= h + 2 pad_h"),      # 4 > 1 + 2
                ((k, x, wb, but(w=1, c_in=8, kw=5, pad_w=1), 32), b"kw <= w + 2 pad_w"),
                ((k, x, wb, but(n_img=2), 32), b"n_img * c_in * h * w"), ((k, x, wb, but(h=4), 32), b"n_img * c_in * h * w"),
                ((k, x, wb, but(c_out=3), 32), b"c_out * c_in * kh * kw"),
                ((k, x, wb, but(kw=2, pad_w=0), 32), b"c_out * c_in * kh * kw"),
                ((k, x, xp, ok, 32), b"plain uploaded batch"),                                  # w in pair rows
                ((k, x, wb, ok, 0), b"e_bits"), ((k, x, wb, ok, 65), b"e_bits"),
                ((k, wide, wb, ok, 32), b"ciphertext width mismatch"),
                ((k, pair_other, wb, ok, 32), b"different key"), ((k, mont_other, wb, ok, 32), b"different key"),
                ((k, x, wb, but(n_img=1 << 40, c_in=1 << 40), 32), b"size_t"),                  # a size product beyond size_t
                ((k, x, wb, but(c_out=1 << 62), 32), b"size_t"), ((k, x, wb, but(n_img=1 << 62, c_out=1 << 3), 32), b"size_t")]
            for args, text in invalid:
                assert call(*args) == -1, args
                assert text in L.pgpu_last_error() and not out.value, (args, L.pgpu_last_error())
            assert L.pgpu_batch_ct_conv2d(k, x, wb, ctypes.byref(cshape(ok)), 32, None) == -1 and b"null" in L.pgpu_last_error()
            # the masked table-gather policy: refused, and the text says why
            assert L.pgpu_set_table_gather_policy(1) == 0
            try:
                assert call(k, x, wb, ok, 32) == -3
                err = L.pgpu_last_error()
                assert b"conv2d" in err and b"masked" in err and b"digits of the plaintext filters" in err and not out.value
            finally:
                L.pgpu_set_table_gather_policy(0)
            # a key class without pair rows
            p4, q4, _ = key_case(4096, False)
            pk4 = engine.PublicKey(p4 * q4, 4096)
            assert call(pk4._h, R.up([3, 5], 128), R.up([1, 2], 1), (1, 2, 1, 1, 1, 1, 1, 1, 1, 0, 0), 32) == -3
            assert b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0    # nothing was launched
        finally:
            L.pgpu_set_timing(0)
        assert R.down(conv(c, x, wb, ok, 32)) == expect(xs, wt, c.nsq, ok)
    finally:
        R.close()


_NO_PAIR_ROWS = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
pk = pa.PublicKey(p * q, 2048, hs=hs)
R = Res()
x, w = R.up([3, 5, 7, 9], 64), R.up([1, 2], 1)
out = ctypes.c_void_p()
shape = _capi.Conv2dShape(2, 1, 1, 2, 1, 1, 2, 1, 1, 0, 0)
rc = R.L.pgpu_batch_ct_conv2d(pk._h, x, w, ctypes.byref(shape), 32, ctypes.byref(out))
err = R.L.pgpu_last_error()
print("rc", rc, err.decode())
R.close()
sys.exit(0 if rc == -3 and b"conv2d: key has no pair form" in err and not out.value else 1)
"""

_STALE = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
nsq = (p * q) ** 2
R = Res()
L = R.L
old_key = pa.PublicKey(p * q, 2048, hs=hs)
old_x, old_w = R.up([3, 5, 7, 9], 64), R.up([2, 3], 1)
L.pgpu_shutdown()                      # the pool the key and the batches were created under is gone
pa.initialize()
new_key = pa.PublicKey(p * q, 2048, hs=hs)
new_x, new_w = R.up([3, 5, 7, 9], 64), R.up([2, 3], 1)
out = ctypes.c_void_p()
shape = _capi.Conv2dShape(2, 1, 1, 2, 1, 1, 2, 1, 1, 0, 0)      # two sequences of two, one kernel of two: a dot product each
ok = True
for key, x, w in ((old_key, new_x, new_w), (new_key, old_x, new_w), (new_key, new_x, old_w)):
    rc = L.pgpu_batch_ct_conv2d(key._h, x, w, ctypes.byref(shape), 2, ctypes.byref(out))
    print("rc", rc, L.pgpu_last_error().decode())
    ok = ok and rc == -1 and b"shut down" in L.pgpu_last_error() and not out.value
rc = L.pgpu_batch_ct_conv2d(new_key._h, new_x, new_w, ctypes.byref(shape), 2, ctypes.byref(out))
ok = ok and rc == 0 and bool(out.value)
if out.value:
    got = R.down(out)
    L.pgpu_batch_destroy(out)
    ok = ok and got == [3 ** 2 * 5 ** 3 % nsq, 7 ** 2 * 9 ** 3 % nsq]
    print("conv2d", got)
L.pgpu_batch_destroy(new_x)
L.pgpu_batch_destroy(new_w)
sys.exit(0 if ok else 1)
"""


def test_refused_without_pair_rows(engine):
    """PGPU_PAIR_ROWS=0 keeps resident ciphertexts as Montgomery-form words: no pair form, PGPU_ERR_UNSUPPORTED (own
    process: the switch is read once)"""
    env = dict(os.environ, PGPU_PAIR_ROWS="0")
    r = subprocess.run([sys.executable, "-c", _NO_PAIR_ROWS, ROOT], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


def test_stale_handles_are_refused(engine):
    """a key or a batch created under a device pool that has been shut down: PGPU_ERR_INVALID_PARAM, *out untouched (own
    process: the pool of the test session stays up)"""
    r = subprocess.run([sys.executable, "-c", _STALE, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


def fold_launches(s):
    n = 0
    while s > 1:
        s = (s + 1) // 2
        n += 1
    return n


def test_timing_record(engine, knobs):
    """every launch of a call is kind 13; passes * (table build + multi-exponentiation + ceil(log2 S) fold launches) of
    them under a forced plan"""
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(31)
    e_bits = 13
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(sizes(BIG)[0])], rng)      # pair rows already: no conversion launch
        xs = R.down(x)
        wt = rand_filter(rng, BIG, e_bits)
        wb = R.up(wt, 1)
        want = expect(xs, wt, c.nsq, BIG)
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        pw, ps, pt, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert L.pgpu_set_timing(1) == 0
        try:
            for forced in ((4, 2, 5), (4, 1, 1), (6, 5, 18), (1, 2, 2), (3, 5, 3)):
                knobs(*forced)
                assert L.pgpu_ct_conv2d_plan(2048, ctypes.byref(cshape(BIG)), e_bits, ctypes.byref(pw), ctypes.byref(ps), ctypes.byref(pt),
                                             ctypes.byref(tb), ctypes.byref(pr)) == 0
                assert (pw.value, pt.value, ps.value) == forced
                passes = -(-BIG[0] // pt.value)
                launches = passes * (2 + fold_launches(ps.value))
                assert launches <= 64
                assert L.pgpu_synchronize() == 0
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)            # drop what earlier calls left
                y = conv(c, x, wb, BIG, e_bits)
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)        # (before the download, which launches a conversion)
                assert n == launches, (forced, n, launches)
                assert all(kinds[i] == KIND_CONV and ms[i] > 0 for i in range(n))
                assert R.down(y) == want
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_key_width_off_the_classes(engine, knobs):
    """1124 bits: the (4,18) rows of the 2048-bit class under a modulus far narrower than the class; the plan's knobs,
    then tiles of 2 images over 5 tap slices"""
    from test_gpu_key_widths import PAIR_WIDTHS, Key
    bits = 1124
    assert bits in PAIR_WIDTHS
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 13)
    try:
        x, m = K.fresh(rng, sizes(BIG)[0])
        xs = R.down(x)
        wt = rand_filter(rng, BIG, 13)
        wb = R.up(wt, 1)
        want = expect(xs, wt, K.nsq, BIG)
        plain = [sum(m[e] * wt[k] for e, k in row) % K.n for row in live_taps(BIG)]
        for forced in ((None, None, None), (None, 2, 5)):
            knobs(*forced)
            y = R.op(L.pgpu_batch_ct_conv2d, K.pk._h, x, wb, ctypes.byref(cshape(BIG)), 13)
            assert L.pgpu_batch_count(y) == 240 and L.pgpu_batch_row_limbs(y) == 2 * K.l2
            assert R.down(y) == want, forced
            assert K.decrypt(y) == plain, forced
        knobs()
    finally:
        K.close()


def test_python_conv2d(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(3)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    n_img, c_in, h, w, c_out, kh, kw = 2, 2, 4, 3, 3, 2, 3
    m = [rng.randrange(1 << 40) for _ in range(n_img * c_in * h * w)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    nest = lambda flat, a, b, cc, d: [[[[flat[((i * b + j) * cc + k) * d + l] for l in range(d)] for k in range(cc)] for j in range(b)] for i in range(a)]  # noqa: E731,E741
    x = nest(ct, n_img, c_in, h, w)
    wt = [rng.getrandbits(20) for _ in range(c_out * c_in * kh * kw)]
    wn = nest(wt, c_out, c_in, kh, kw)

    def plain(shape):
        return [sum(m[e] * wt[k] for e, k in row) % n for row in live_taps(shape)]

    def check(y, shape):
        oh, ow = out_size(shape)
        assert len(y) == n_img and all(len(f) == c_out and all(len(r) == oh and all(len(v) == ow for v in r) for r in f) for f in y)
        assert sk.decrypt([v for img in y for f in img for r in f for v in r]) == plain(shape)
    check(pk.conv2d(x, wn), (n_img, c_in, h, w, c_out, kh, kw, 1, 1, 0, 0))
    check(pk.conv2d(x, wn, stride=2, padding=1), (n_img, c_in, h, w, c_out, kh, kw, 2, 2, 1, 1))
    check(pk.conv2d(x, wn, stride=(2, 1), padding=(1, 2)), (n_img, c_in, h, w, c_out, kh, kw, 2, 1, 1, 2))
    check(pk.conv2d(x, wn, stride=[1, 3], padding=(0, 1), e_bits=24), (n_img, c_in, h, w, c_out, kh, kw, 1, 3, 0, 1))
    with pytest.raises(RuntimeError, match="conv2d error: Size mismatch!"):
        pk.conv2d(x, [[[[1, 2, 3], [4, 5, 6]]]])                      # one input channel where x has two
    with pytest.raises(RuntimeError, match="conv2d error: Size mismatch!"):
        pk.conv2d([ct], wn)                                           # not [n_img][C_in][H][W]
    with pytest.raises(RuntimeError, match="conv2d error: Size mismatch!"):
        pk.conv2d(x[:1] + [[x[1][0]]], wn)                            # a ragged batch
    with pytest.raises(RuntimeError, match="conv2d error: negative weights have no encoding"):
        pk.conv2d(x, nest([-1] + wt[1:], c_out, c_in, kh, kw))
    with pytest.raises(RuntimeError, match="conv2d error: the padding must be smaller than the kernel"):
        pk.conv2d(x, wn, padding=2)
    with pytest.raises(RuntimeError, match="conv2d error: the stride must be positive"):
        pk.conv2d(x, wn, stride=0)
    with pytest.raises(RuntimeError, match="conv2d error: the kernel exceeds the padded image"):
        pk.conv2d(x, nest(list(range(5 * 3)) * (c_out * c_in), c_out, c_in, 5, 3))
    with pytest.raises(RuntimeError, match="stride must be a non-negative int or a pair"):
        pk.conv2d(x, wn, stride=(1, 2, 3))
