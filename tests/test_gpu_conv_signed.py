"""The signed-weight encrypted 2-D convolution on resident ciphertexts (pgpu_batch_ct_conv2d_signed;
csrc/hensel_conv_signed.hpp) on the GPU:
    out[n][co][oy][ox] = prod_{ci,ky,kx} x[n][ci][oy*sh + ky - ph][ox*sw + kx - pw]^w[co][ci][ky][kx] mod n^2,
w two's complement in e_bits bits, a tap outside the image left out -- held bit-identical to Python's pow with signed
exponents (a negative one through pow(x, -1, n^2)) at 1024, 2048, 3072 bits and one width off the classes (2051).  The
shapes are those of tests/test_conv_model.py.  Further, bit for bit: sub(conv2d(x, W+), conv2d(x, W-)) on the same handles,
pgpu_batch_ct_spmv_signed in the spmv formulation of the same map, the signed matvec and the transposed signed matmul a
convolution degenerates to, the unsigned conv2d on non-negative weights with e_bits one bit wider; the 240-output shape
under every forced window x slices x tiles; a short last pass on more slices than the full passes; every e_bits of the
signed matvec's tests, rows one word wider than e_bits needs, the edge weights, garbage above e_bits, negative weights on
padded taps; two layers chained through CRT decrypt against torch.nn.functional.conv2d; two lanes at once; a non-unit in
the last tile; the host-side refusals, the timing record and the Python keyword."""
import ctypes
import json
import os
import random
import threading

import numpy as np
import pytest

from test_conv_model import BIG, SHAPES, out_size
from test_gpu_conv import cshape, fold_launches, live_taps, sizes
from test_gpu_matvec_signed import INVALID, KIND_INVERT, NOT_INVERTIBLE, UNSUPPORTED, Case
from test_gpu_pair_rows import Res, key_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [1024, 2048, 3072, 2051]
KNOBS = ("PGPU_CONV_WINDOW", "PGPU_CONV_TILE", "PGPU_CONV_SLICES")
KIND_CONV, KIND_SPMV = 13, 9
E_BITS = [1, 2, 13, 32, 63, 64, 65, 70]


@pytest.fixture
def knobs(monkeypatch):
    for name in KNOBS + ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_SPMV_WINDOW", "PGPU_SPMV_CHUNK", "PGPU_MATMUL_WINDOW",
                         "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES", "PGPU_INVERT_CHUNK", "PGPU_INVERT_WIDE"):
        monkeypatch.delenv(name, raising=False)

    def force(w=None, t=None, s=None):
        for name, v in zip(KNOBS, (w, t, s)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


def up_w(c, wt, e_bits, words=None, garbage=None):
    """signed weights as a plain uploaded batch: two's complement in e_bits bits, optional garbage in the stored bits above"""
    ew = words or (e_bits + 63) // 64
    flat = [v & ((1 << e_bits) - 1) for v in wt]
    if garbage is not None:
        flat = [(v | (garbage.getrandbits(64 * ew) << e_bits)) & ((1 << (64 * ew)) - 1) for v in flat]
    return c.R.up(flat, ew)


def conv_s(c, x, wb, shape, e_bits):
    return c.R.op(c.L.pgpu_batch_ct_conv2d_signed, c.pk._h, x, wb, ctypes.byref(cshape(shape)), e_bits)


def conv_u(c, x, wb, shape, e_bits):
    return c.R.op(c.L.pgpu_batch_ct_conv2d, c.pk._h, x, wb, ctypes.byref(cshape(shape)), e_bits)


def expect(xs, wt, nsq, shape, xinv=None):
    """the definition with Python's pow on signed exponents; the inverses once per element"""
    xinv = xinv or [pow(x, -1, nsq) for x in xs]
    out = []
    for row in live_taps(shape):
        acc = 1
        for e, k in row:
            if wt[k]:
                acc = acc * (pow(xs[e], wt[k], nsq) if wt[k] > 0 else pow(xinv[e], -wt[k], nsq)) % nsq
        out.append(acc)
    return out


def rand_filter(rng, n_w, e_bits):
    top = 1 << (e_bits - 1)
    return [rng.randrange(-top, top) for _ in range(n_w)]


def e_bits_of(shape):
    n_x, n_w, n_out = sizes(shape)
    return 32 if n_out * shape[1] * shape[5] * shape[6] < 1000 else 13


def spmv_signed_formulation(c, x, wt, shape, e_bits):
    """CSR rows of the live taps of every output, column numbers into x, the signed weights replicated"""
    rows = live_taps(shape)
    rp = np.cumsum([0] + [len(r) for r in rows]).astype(np.uint64)
    ci = np.array([e for r in rows for e, _ in r], dtype=np.uint32)
    wb = up_w(c, [wt[k] for r in rows for _, k in r], e_bits)
    return c.R.op(c.L.pgpu_batch_ct_spmv_signed, c.pk._h, x, rp.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p), wb,
                  len(rows), e_bits)


@pytest.mark.parametrize("bits", BITS)
def test_exact_at_every_shape_and_against_the_other_routes(engine, knobs, bits):
    """x from a resident DJN encrypt and as uploaded plain ciphertext words; the plan the policy picks; x unchanged; the
    composed route, the spmv formulation, the signed matvec and the transposed signed matmul on the same handles"""
    c = Case(engine, bits)
    L, R = c.L, c.R
    rng = random.Random(bits)
    try:
        for shape in SHAPES:
            n_x, n_w, n_out = sizes(shape)
            e_bits = e_bits_of(shape)
            x = c.encrypt([rng.randrange(c.n) for _ in range(n_x)], rng)
            xs = R.down(x)
            wt = rand_filter(rng, n_w, e_bits)
            wt[0] = -abs(wt[0]) - 1 if e_bits > 1 else -1                           # at least one negative weight
            wb = up_w(c, wt, e_bits)
            want = expect(xs, wt, c.nsq, shape)
            y = conv_s(c, x, wb, shape, e_bits)
            assert L.pgpu_batch_count(y) == n_out and L.pgpu_batch_row_limbs(y) > 0 and L.pgpu_batch_lane(y) == L.pgpu_batch_lane(x)
            assert R.down(y) == want, shape
            assert R.down(x) == xs, shape                                           # x is left unchanged
            assert R.down(conv_s(c, c.up(xs), wb, shape, e_bits)) == want, shape    # plain ciphertext words
            # sub(conv2d(x, W+), conv2d(x, W-)) on the same handles: |w| < 2^(e_bits - 1) but for -2^(e_bits - 1), e_bits bits
            plus, minus = R.up([max(v, 0) for v in wt], 1), R.up([max(-v, 0) for v in wt], 1)
            composed = R.op(L.pgpu_batch_ct_sub, c.pk._h, conv_u(c, x, plus, shape, e_bits), conv_u(c, x, minus, shape, e_bits))
            assert R.down(composed) == want, shape
            assert R.down(spmv_signed_formulation(c, x, wt, shape, e_bits)) == want, shape
            n_img, c_in, h, w, c_out, kh, kw = shape[:7]
            if (kh, kw) == (h, w) and n_img == 1 and shape[9:] == (0, 0):           # kernel equal to the image: the matvec
                assert R.down(c.matvec(x, wb, c_out, e_bits)) == want
            if (kh, kw) == (1, 1) and n_img == 1:                                   # 1x1 kernel: x is [cols = C_in][n_vec = H*W]
                assert R.down(c.matmul(x, wb, h * w, c_out, e_bits, 1)) == want
            # non-negative weights: the unsigned call, with e_bits one bit wider here
            pos = [abs(v) % (1 << (e_bits - 1)) if e_bits > 1 else 0 for v in wt]
            if e_bits > 1:
                assert R.down(conv_s(c, x, R.up(pos, 1), shape, e_bits)) == R.down(conv_u(c, x, R.up(pos, 1), shape, e_bits - 1)), shape
            R.close()
    finally:
        R.close()


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("bits", BITS)
def test_forced_windows_slices_and_tiles(engine, knobs, bits, w, big_case):
    """the 240-output shape over 18 taps: slices 1, 2, 5 (does not divide 18), 18 x tiles 1, 2 (passes of 2, 2 and 1), 5"""
    c, xs, wt, want = big_case(engine, bits)
    try:
        x, wb = c.up(xs), up_w(c, wt, 13)
        for s in (1, 2, 5, 18):
            for t in (1, 2, 5):
                knobs(w, t, s)
                assert c.R.down(conv_s(c, x, wb, BIG, 13)) == want, (w, s, t)
        knobs()
    finally:
        c.R.close()


@pytest.fixture(scope="module")
def big_case():
    """per key width: units, a signed 13-bit filter and the reference of the 240-output shape, computed once"""
    cache = {}

    def get(engine, bits):
        if bits not in cache:
            c = Case(engine, bits)
            rng = random.Random(bits + 1)
            xs = c.units(rng, sizes(BIG)[0])
            wt = rand_filter(rng, sizes(BIG)[1], 13)
            cache[bits] = (c, xs, wt, expect(xs, wt, c.nsq, BIG))
        return cache[bits]
    return get


def test_last_pass_on_more_slices_than_a_full_pass(engine, knobs):
    """3072 bits, 9 images of 11 x 11 under 8 filters of 4 x 4 -> 512 outputs per image over 16 taps, in tiles of 8, no
    forced slices: a full pass runs on 2 slices, the last pass of one image on 4, inside a partial block sized by the
    larger count.  Weights of 2 bits: -2 .. 1"""
    bits, e_bits, tile = 3072, 2, 8
    c = Case(engine, bits)
    rng = random.Random(bits + 5)
    shape = (9, 1, 11, 11, 8, 4, 4, 1, 1, 0, 0)
    n_x, n_w, n_out = sizes(shape)
    ps, pt = ctypes.c_int(), ctypes.c_size_t()

    def plan(n_img):
        sh = cshape((n_img,) + shape[1:])
        assert c.L.pgpu_ct_conv2d_signed_plan(bits, ctypes.byref(sh), e_bits, None, ctypes.byref(ps), ctypes.byref(pt), None, None) == 0
        return ps.value, pt.value
    try:
        knobs(None, tile, None)
        full, one, whole = plan(tile), plan(1), plan(9)
        print(f"signed conv2d plan, {bits} bits, tile {tile}: slices {full[0]} with {tile} images, {one[0]} with one, {whole[0]} with 9")
        assert full == (2, tile) and one == (4, 1) and whole == (2, tile)
        xs = c.units(rng, n_x)
        wt = rand_filter(rng, n_w, e_bits)
        tab = [{e: pow(x, e, c.nsq) for e in (-2, -1, 1)} for x in xs]      # pow once per (x, weight)
        want = []
        for row in live_taps(shape):
            acc = 1
            for e, k in row:
                if wt[k]:
                    acc = acc * tab[e][wt[k]] % c.nsq
            want.append(acc)
        assert c.R.down(conv_s(c, c.up(xs), up_w(c, wt, e_bits), shape, e_bits)) == want
    finally:
        c.R.close()


@pytest.mark.parametrize("e_bits", E_BITS)
def test_widths_edge_weights_and_ignored_bits(engine, knobs, e_bits):
    """5 filters of 8 taps padded on both axes: all 0, all -1, all -2^(e-1), all 2^(e-1) - 1, random; then rows one word
    wider than e_bits needs with garbage in every stored bit above e_bits; 70: a window starting at bit 64"""
    c = Case(engine, 2048)
    rng = random.Random(e_bits + 2)
    shape = (1, 2, 4, 3, 5, 2, 2, 1, 1, 1, 1)
    n_x, n_w, n_out = sizes(shape)
    taps, top = 8, 1 << (e_bits - 1)
    try:
        xs = c.units(rng, n_x)
        xinv = [pow(v, -1, c.nsq) for v in xs]
        x = c.up(xs)
        oh, ow = out_size(shape)
        wt = [0] * taps + [-1] * taps + [-top] * taps + [top - 1] * taps + rand_filter(rng, taps, e_bits)
        want = expect(xs, wt, c.nsq, shape, xinv)
        assert all(want[k] == 1 for k in range(oh * ow))                       # an all-zero filter: the ciphertext 1
        assert any(len(r) < 8 for r in live_taps(shape))                       # negative weights fall into the padding
        ew = (e_bits + 63) // 64
        for win in (None, 1, 3, 6):
            knobs(win, None, None)
            assert c.R.down(conv_s(c, x, up_w(c, wt, e_bits), shape, e_bits)) == want, win
            assert c.R.down(conv_s(c, x, up_w(c, wt, e_bits, ew + 1, rng), shape, e_bits)) == want, win      # garbage, a wider row
        if 64 * ew > e_bits:
            assert c.R.down(conv_s(c, x, up_w(c, wt, e_bits, ew, rng), shape, e_bits)) == want                 # garbage inside the row
        knobs()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_two_chained_layers_then_decrypt(engine, knobs, bits):
    """the second signed layer takes the first one's result as it is; Dec mod n against torch's conv2d on int64 CPU
    tensors: plaintexts below 2^20, |weights| below 2^12, 18 and 12 taps -- |sums| stay below 2^20 * 2^12 * 18 * 2^12 * 12 < 2^52"""
    import torch
    import torch.nn.functional as F
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    s1 = (2, 2, 6, 5, 3, 3, 3, 1, 1, 1, 1)                # -> [2][3][6][5]
    s2 = (2, 3, 6, 5, 2, 2, 2, 2, 2, 0, 1)                # -> [2][2][3][3]
    try:
        m = [rng.randrange(1 << 20) for _ in range(sizes(s1)[0])]
        w1, w2 = rand_filter(rng, sizes(s1)[1], 13), rand_filter(rng, sizes(s2)[1], 13)
        tm = torch.tensor(m, dtype=torch.int64).reshape(2, 2, 6, 5)
        t1 = F.conv2d(tm, torch.tensor(w1, dtype=torch.int64).reshape(3, 2, 3, 3), stride=(1, 1), padding=(1, 1))
        t2 = F.conv2d(t1, torch.tensor(w2, dtype=torch.int64).reshape(2, 3, 2, 2), stride=(2, 2), padding=(0, 1))
        assert (1 << 20) * (1 << 12) * 18 * (1 << 12) * 12 < 1 << 63 and int(t1.min()) < 0 and int(t2.min()) < 0
        x = c.encrypt(m, rng)
        xs = R.down(x)
        y = conv_s(c, x, up_w(c, w1, 13), s1, 13)
        ys = expect(xs, w1, c.nsq, s1)
        assert R.down(y) == ys
        z = conv_s(c, y, up_w(c, w2, 13), s2, 13)         # the first layer's result as it is
        assert R.down(z) == expect(ys, w2, c.nsq, s2)
        assert c.decrypt(z) == [int(v) % c.n for v in t2.flatten().tolist()]
        assert c.decrypt(y) == [int(v) % c.n for v in t1.flatten().tolist()]
    finally:
        R.close()


def test_two_lanes_at_once(engine, knobs):
    """two threads on different batch lanes, each with its own x and shape, the filters uploaded by the main thread; tiles
    of 2 images over 3 tap slices; three calls in a row per thread"""
    c = Case(engine, 2048)
    L = c.L
    rng = random.Random(12)
    results, errors = {}, []
    shapes = {1: BIG, 2: SHAPES[2]}
    wts = {lane: rand_filter(rng, sizes(sh)[1], 13) for lane, sh in shapes.items()}
    xss = {lane: c.units(rng, sizes(sh)[0]) for lane, sh in shapes.items()}
    knobs(None, 2, 3)

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            x = R.up(xss[lane], 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for it in range(3):
                y = R.op(L.pgpu_batch_ct_conv2d_signed, c.pk._h, x, ws[lane], ctypes.byref(cshape(shapes[lane])), 13)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = R.down(y)
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    try:
        ws = {lane: up_w(c, wts[lane], 13) for lane in shapes}         # lane of the main thread: ordered in by events
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


def test_a_non_unit_in_the_last_tile_is_refused_after_the_inversion(engine, knobs):
    """tile 2 over 5 images: the non-unit belongs to the last pass.  The inversion runs over all of x before the first
    pass: PGPU_ERR_NOT_INVERTIBLE, *out null, no launch of kind PGPU_KERNEL_CONV recorded; the next call on the lane is exact"""
    c = Case(engine, 2048)
    rng = random.Random(80)
    L, R = c.L, c.R
    shape = (5, 1, 3, 3, 2, 2, 2, 1, 1, 0, 0)
    n_x, n_w, n_out = sizes(shape)
    try:
        xs = c.units(rng, n_x)
        wt = rand_filter(rng, n_w, 32)
        wb = up_w(c, wt, 32)
        want = expect(xs, wt, c.nsq, shape)
        x = c.up(xs)
        out = ctypes.c_void_p()
        kinds, forms, ms = (ctypes.c_int * 256)(), (ctypes.c_int * 256)(), (ctypes.c_double * 256)()
        knobs(None, 2, None)
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            for bad in (c.p, c.n, 0):
                bad_xs = list(xs)
                bad_xs[4 * 9 + 1] = bad                                           # image 4: the last pass
                xb = c.up(bad_xs)
                L.pgpu_timing_collect_ex(kinds, forms, ms, 256)                   # drop what earlier calls left
                assert L.pgpu_batch_ct_conv2d_signed(c.pk._h, xb, wb, ctypes.byref(cshape(shape)), 32, ctypes.byref(out)) == NOT_INVERTIBLE
                assert not out.value and b"unit" in L.pgpu_last_error()
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 256)
                seen = [kinds[i] for i in range(n)]
                assert KIND_INVERT in seen and KIND_CONV not in seen, (bad == c.p, seen)
                assert R.down(conv_s(c, x, wb, shape, 32)) == want                # the lane stays usable
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_refusals_are_host_side(engine, knobs):
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(9)
    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    ok = (1, 2, 3, 4, 2, 2, 3, 1, 1, 1, 1)                # 24 ciphertexts, 24 taps in all
    try:
        xs = c.units(rng, 24)
        x = c.up(xs)
        xp = c.encrypt(list(range(1, 25)), rng)
        wt = rand_filter(rng, 24, 32)
        wb = up_w(c, wt, 32)
        other = engine.PublicKey(int(json.load(open(os.path.join(ROOT, "tests", "golden", "aggregate_refusals.json")))["other_n"]["2048"], 16), 2048)
        pair_other = R.op(L.pgpu_batch_ct_add, other._h, c.up(xs), c.up(xs))
        wide = R.up(xs, 2 * c.nw + 1)
        out = ctypes.c_void_p()
        k = c.pk._h

        def call(key, xb, wbatch, shape, e_bits):
            return L.pgpu_batch_ct_conv2d_signed(key, xb, wbatch, ctypes.byref(cshape(shape)) if shape else None, e_bits, ctypes.byref(out))

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
                ((k, x, wb, but(h=1, c_in=6, kh=4, pad_h=1), 32), b"kh <= h + 2 pad_h"),
                ((k, x, wb, but(w=1, c_in=8, kw=5, pad_w=1), 32), b"kw <= w + 2 pad_w"),
                ((k, x, wb, but(n_img=2), 32), b"n_img * c_in * h * w"), ((k, x, wb, but(h=4), 32), b"n_img * c_in * h * w"),
                ((k, x, wb, but(c_out=3), 32), b"c_out * c_in * kh * kw"),
                ((k, x, xp, ok, 32), b"plain uploaded batch"),                                  # w in pair rows
                ((k, x, wb, ok, 0), b"e_bits"), ((k, x, wb, ok, 65), b"e_bits"),
                ((k, wide, wb, ok, 32), b"ciphertext width mismatch"),
                ((k, pair_other, wb, ok, 32), b"different key"),
                ((k, x, wb, but(n_img=1 << 40, c_in=1 << 40), 32), b"size_t"),
                ((k, x, wb, but(c_out=1 << 62), 32), b"size_t")]
            for args, text in invalid:
                assert call(*args) == INVALID, args
                assert text in L.pgpu_last_error() and not out.value, (args, L.pgpu_last_error())
            assert L.pgpu_batch_ct_conv2d_signed(k, x, wb, ctypes.byref(cshape(ok)), 32, None) == INVALID and b"null" in L.pgpu_last_error()
            # the masked table-gather policy: refused, and the text says why
            assert L.pgpu_set_table_gather_policy(1) == 0
            try:
                assert call(k, x, wb, ok, 32) == UNSUPPORTED
                err = L.pgpu_last_error()
                assert b"signed conv2d" in err and b"masked" in err and b"digits of the plaintext filters" in err and not out.value
            finally:
                L.pgpu_set_table_gather_policy(0)
            # a key class without pair rows
            p4, q4, _ = key_case(4096, False)
            pk4 = engine.PublicKey(p4 * q4, 4096)
            assert call(pk4._h, R.up([3, 5], 128), R.up([1, 2], 1), (1, 2, 1, 1, 1, 1, 1, 1, 1, 0, 0), 32) == UNSUPPORTED
            assert b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0    # nothing was launched
        finally:
            L.pgpu_set_timing(0)
        assert R.down(conv_s(c, x, wb, ok, 32)) == expect(xs, wt, c.nsq, ok)
    finally:
        R.close()


def test_timing_record(engine, knobs):
    """the record of a call reads INVERT launches first, then passes * (table build + multi-exponentiation +
    ceil(log2 S) fold launches) of kind 13, under forced plans"""
    c, xs, wt, want = Case(engine, 2048), None, None, None
    L, R = c.L, c.R
    rng = random.Random(31)
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(sizes(BIG)[0])], rng)      # pair rows already: no conversion launch
        xs = R.down(x)
        wt = rand_filter(rng, sizes(BIG)[1], 13)
        wb = up_w(c, wt, 13)
        want = expect(xs, wt, c.nsq, BIG)
        kinds, forms, ms = (ctypes.c_int * 128)(), (ctypes.c_int * 128)(), (ctypes.c_double * 128)()
        pw, ps, pt = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        n_inv = ctypes.c_int()
        assert L.pgpu_ct_negate_plan(2048, sizes(BIG)[0], None, None, ctypes.byref(n_inv), None) == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            for forced in ((4, 2, 5), (4, 1, 1), (6, 5, 18), (1, 2, 2), (3, 5, 3)):
                knobs(*forced)
                assert L.pgpu_ct_conv2d_signed_plan(2048, ctypes.byref(cshape(BIG)), 13, ctypes.byref(pw), ctypes.byref(ps), ctypes.byref(pt),
                                                    None, None) == 0
                assert (pw.value, pt.value, ps.value) == forced
                passes = -(-BIG[0] // pt.value)
                launches = passes * (2 + fold_launches(ps.value))
                assert L.pgpu_synchronize() == 0
                L.pgpu_timing_collect_ex(kinds, forms, ms, 128)           # drop what earlier calls left
                y = conv_s(c, x, wb, BIG, 13)
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 128)       # (before the download, which launches a conversion)
                seen = [kinds[i] for i in range(n)]
                assert seen.count(KIND_INVERT) == n_inv.value, (forced, seen)     # forward passes and walks back
                last = max(i for i in range(n) if seen[i] == KIND_INVERT)         # (the grand total's conversions lie between them)
                assert KIND_CONV not in seen[:last]
                assert seen[last + 1:] == [KIND_CONV] * launches, (forced, seen)
                assert all(ms[i] > 0 for i in range(n))
                assert R.down(y) == want
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_python_keyword(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(3)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    n_img, c_in, h, w, c_out, kh, kw = 2, 2, 4, 3, 3, 2, 3
    m = [rng.randrange(1 << 40) for _ in range(n_img * c_in * h * w)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    nest = lambda flat, a, b, cc, d: [[[[flat[((i * b + j) * cc + k) * d + l] for l in range(d)] for k in range(cc)] for j in range(b)] for i in range(a)]  # noqa: E731,E741
    x = nest(ct, n_img, c_in, h, w)
    wt = rand_filter(rng, c_out * c_in * kh * kw, 20)
    wt[0], wt[1] = -(1 << 19), (1 << 19) - 1
    wn = nest(wt, c_out, c_in, kh, kw)

    def check(y, shape):
        assert sk.decrypt([v for img in y for f in img for r in f for v in r]) == [sum(m[e] * wt[k] for e, k in row) % n for row in live_taps(shape)]
    check(pk.conv2d(x, wn, signed=True), (n_img, c_in, h, w, c_out, kh, kw, 1, 1, 0, 0))
    check(pk.conv2d(x, wn, stride=(2, 1), padding=(1, 2), signed=True), (n_img, c_in, h, w, c_out, kh, kw, 2, 1, 1, 2))
    check(pk.conv2d(x, wn, stride=2, padding=1, e_bits=24, signed=True), (n_img, c_in, h, w, c_out, kh, kw, 2, 2, 1, 1))
    flat = lambda y: [v for img in y for f in img for r in f for v in r]      # noqa: E731
    assert flat(pk.conv2d(x, wn, signed=True)) == flat(pk.conv2d(x, wn, e_bits=20, signed=True))      # the default width
    with pytest.raises(RuntimeError, match="conv2d error: negative weights have no encoding"):
        pk.conv2d(x, wn)                                              # signed=False: today's behaviour
    pos = nest([abs(v) for v in wt], c_out, c_in, kh, kw)
    assert flat(pk.conv2d(x, pos)) == flat(pk.conv2d(x, pos, signed=True))
