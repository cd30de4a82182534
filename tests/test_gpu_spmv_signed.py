"""The signed-weight encrypted sparse matrix-vector product on resident ciphertexts (pgpu_batch_ct_spmv_signed;
csrc/hensel_spmv_signed.hpp) on the GPU:
    out[i] = prod_{ row_ptr[i] <= t < row_ptr[i+1] } x[col_idx[t]]^w[t] mod n^2,   w two's complement in e_bits bits,
held bit-identical to Python's pow with signed exponents (a negative one through pow(x, -1, n^2)) for the 1024-, 2048-
and 3072-bit key classes.  The ragged CSR builders are those of tests/test_gpu_spmv.py: empty rows, rows longer than the
chunk (fold levels), forced windows 1..6 x chunks.  Further: a column named twice with weights a and -a gives the
ciphertext 1 exactly; the e_bits values and edge weights of the signed convolution's tests; sub(spmv(W+), spmv(W-)) and the
signed matvec on a dense row, bit for bit; a non-unit in an unreferenced column refuses the call; the host-side refusals,
the launch kinds and the Python keyword."""
import ctypes
import json
import os
import random

import numpy as np
import pytest

from test_gpu_matvec_signed import INVALID, KIND_INVERT, NOT_INVERTIBLE, UNSUPPORTED, Case
from test_gpu_pair_rows import key_case
from test_gpu_spmv import csr

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [1024, 2048, 3072]
KIND_SPMV = 9
E_BITS = [1, 2, 13, 32, 63, 64, 65, 70]


@pytest.fixture
def knobs(monkeypatch):
    names = ("PGPU_SPMV_WINDOW", "PGPU_SPMV_CHUNK")
    for name in names + ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_INVERT_CHUNK", "PGPU_INVERT_WIDE"):
        monkeypatch.delenv(name, raising=False)

    def force(w=None, c=None):
        for name, v in zip(names, (w, c)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


def up_w(c, wt, e_bits, words=None, garbage=None):
    ew = words or (e_bits + 63) // 64
    flat = [v & ((1 << e_bits) - 1) for v in wt]
    if garbage is not None:
        flat = [(v | (garbage.getrandbits(64 * ew) << e_bits)) & ((1 << (64 * ew)) - 1) for v in flat]
    return c.R.up(flat, ew)


def spmv(c, fn, x, row_ptr, col_idx, wb, e_bits):
    rp, ci = np.array(row_ptr, dtype=np.uint64), np.array(col_idx, dtype=np.uint32)
    y = c.R.op(fn, c.pk._h, x, rp.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p), wb, len(row_ptr) - 1, e_bits)
    rp[:] = 0                                                  # row_ptr and col_idx may be reused once the call returns
    ci[:] = 0xFFFFFFFF
    return y


def spmv_s(c, x, row_ptr, col_idx, wb, e_bits):
    return spmv(c, c.L.pgpu_batch_ct_spmv_signed, x, row_ptr, col_idx, wb, e_bits)


def expect(xs, row_ptr, col_idx, wt, nsq, xinv=None):
    xinv = xinv or [pow(x, -1, nsq) for x in xs]
    out = []
    for i in range(len(row_ptr) - 1):
        acc = 1
        for t in range(row_ptr[i], row_ptr[i + 1]):
            if wt[t]:
                j = col_idx[t]
                acc = acc * (pow(xs[j], wt[t], nsq) if wt[t] > 0 else pow(xinv[j], -wt[t], nsq)) % nsq
        out.append(acc)
    return out


def rand_weights(rng, count, e_bits):
    top = 1 << (e_bits - 1)
    return [rng.randrange(-top, top) for _ in range(count)]


@pytest.mark.parametrize("bits", BITS)
def test_ragged_matrix_is_exact(engine, knobs, bits):
    """135 rows over 40 columns, lengths from {0, 1, 2, 3, 7, 40}, first and last row empty: with the default chunk of 4
    rows of 7 are two chains, rows of 40 ten (two fold levels); then one chain, and 33 rows: one past a wavefront at
    (2,19).  x from a resident encrypt; x unchanged; against sub(spmv(W+), spmv(W-)) on the same handles"""
    c = Case(engine, bits)
    L, R = c.L, c.R
    rng = random.Random(bits)
    try:
        cols, e_bits = 40, 12
        x = c.encrypt([rng.randrange(c.n) for _ in range(cols)], rng)
        xs = R.down(x)
        xinv = [pow(v, -1, c.nsq) for v in xs]
        lengths = [0] + [rng.choice((0, 1, 2, 3, 7, 40)) for _ in range(133)] + [0]
        lengths[5], lengths[77] = 40, 7
        for lens in (lengths, [3], [rng.choice((1, 2, 3)) for _ in range(33)]):
            row_ptr, col_idx = csr(rng, lens, cols)
            wt = rand_weights(rng, len(col_idx), e_bits)
            wt[0] = -5
            y = spmv_s(c, x, row_ptr, col_idx, up_w(c, wt, e_bits), e_bits)
            assert L.pgpu_batch_count(y) == len(lens) and L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(x) > 0
            assert L.pgpu_batch_lane(y) == L.pgpu_batch_lane(x)
            got = R.down(y)
            assert got == expect(xs, row_ptr, col_idx, wt, c.nsq, xinv), len(lens)
            assert all(g == 1 for g, m in zip(got, lens) if m == 0)
            plus = spmv(c, L.pgpu_batch_ct_spmv, x, row_ptr, col_idx, R.up([max(v, 0) for v in wt], 1), e_bits)
            minus = spmv(c, L.pgpu_batch_ct_spmv, x, row_ptr, col_idx, R.up([max(-v, 0) for v in wt], 1), e_bits)
            assert R.down(R.op(L.pgpu_batch_ct_sub, c.pk._h, plus, minus)) == got, len(lens)
        assert R.down(x) == xs                                            # x is unchanged
    finally:
        R.close()


@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("bits", BITS)
def test_forced_windows_and_chunks(engine, knobs, bits, w):
    """9 x 20: one row with all 20 columns, one row with a column three times; chunk 2 on 20 entries: four fold levels"""
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    try:
        cols = 20
        xs = c.units(rng, cols)
        xinv = [pow(v, -1, c.nsq) for v in xs]
        x = c.up(xs)
        row_ptr, col_idx = csr(rng, [4, 20, 0, 5, 1, 3, 7, 2, 6], cols, distinct=True)
        full = list(range(cols))
        rng.shuffle(full)                                                 # entries of a row need not be sorted
        col_idx[row_ptr[1]:row_ptr[2]] = full
        col_idx[row_ptr[3]:row_ptr[3] + 5] = [11, 4, 11, 17, 11]         # a column named three times
        for e_bits in (1, 13, 32, 65):
            wt = rand_weights(rng, len(col_idx), e_bits)
            want = expect(xs, row_ptr, col_idx, wt, c.nsq, xinv)
            wb = up_w(c, wt, e_bits)
            for chunk in (1, 2, 3, 64):
                knobs(w, chunk)
                assert c.R.down(spmv_s(c, x, row_ptr, col_idx, wb, e_bits)) == want, (e_bits, w, chunk)
        knobs()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_opposite_weights_on_one_column_cancel(engine, knobs, bits):
    """a column named twice in a row with weights a and -a: the ciphertext 1 exactly, in one chain and across two"""
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    try:
        xs = c.units(rng, 3)
        x = c.up(xs)
        row_ptr, col_idx = [0, 2, 5, 5], [1, 1, 2, 0, 2]
        for e_bits, a in ((13, 1234), (64, (1 << 63) - 1), (70, 1 << 68)):
            wt = [a, -a, -a, 7, a]
            for chunk in (None, 1, 2):
                knobs(None, chunk)
                assert c.R.down(spmv_s(c, x, row_ptr, col_idx, up_w(c, wt, e_bits), e_bits)) == [1, pow(xs[0], 7, c.nsq), 1], (e_bits, chunk)
        knobs()
    finally:
        c.R.close()


@pytest.mark.parametrize("e_bits", E_BITS)
def test_widths_edge_weights_and_ignored_bits(engine, knobs, e_bits):
    """rows of all 0, all -1, all -2^(e-1), all 2^(e-1) - 1, alternating and random weights, an empty row; rows one word
    wider than e_bits needs with garbage in every stored bit above e_bits; 70: a window starting at bit 64"""
    c = Case(engine, 2048)
    rng = random.Random(e_bits + 4)
    cols, top = 9, 1 << (e_bits - 1)
    try:
        xs = c.units(rng, cols)
        xinv = [pow(v, -1, c.nsq) for v in xs]
        x = c.up(xs)
        lens = [5, 5, 5, 5, 6, 0, 7]
        row_ptr, col_idx = csr(rng, lens, cols)
        wt = [0] * 5 + [-1] * 5 + [-top] * 5 + [top - 1] * 5 + [(-top, top - 1)[j % 2] for j in range(6)] + rand_weights(rng, 7, e_bits)
        want = expect(xs, row_ptr, col_idx, wt, c.nsq, xinv)
        assert want[0] == want[5] == 1
        ew = (e_bits + 63) // 64
        for win in (None, 1, 3, 6):
            knobs(win, None)
            assert c.R.down(spmv_s(c, x, row_ptr, col_idx, up_w(c, wt, e_bits), e_bits)) == want, win
            assert c.R.down(spmv_s(c, x, row_ptr, col_idx, up_w(c, wt, e_bits, ew + 1, rng), e_bits)) == want, win
        knobs()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_dense_row_is_the_signed_matvec(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 5)
    try:
        rows, cols, e_bits = 3, 37, 32
        x = c.encrypt([rng.randrange(c.n) for _ in range(cols)], rng)
        wt = rand_weights(rng, rows * cols, e_bits)
        wb = up_w(c, wt, e_bits)
        row_ptr, col_idx = [cols * i for i in range(rows + 1)], list(range(cols)) * rows
        got = c.R.down(spmv_s(c, x, row_ptr, col_idx, wb, e_bits))
        assert got == c.R.down(c.matvec(x, wb, rows, e_bits))
        assert got == expect(c.R.down(x), row_ptr, col_idx, wt, c.nsq)
    finally:
        c.R.close()


def test_a_non_unit_in_an_unreferenced_column_is_refused(engine, knobs):
    """the call inverts every element of x: PGPU_ERR_NOT_INVERTIBLE, *out null, no launch of kind PGPU_KERNEL_SPMV recorded,
    and the next call on the lane is exact"""
    c = Case(engine, 2048)
    rng = random.Random(81)
    L, R = c.L, c.R
    try:
        cols = 12
        xs = c.units(rng, cols)
        row_ptr, col_idx = csr(rng, [3, 0, 4, 2], cols - 1)               # column 11 is never named
        wt = rand_weights(rng, len(col_idx), 32)
        wb = up_w(c, wt, 32)
        want = expect(xs, row_ptr, col_idx, wt, c.nsq)
        out = ctypes.c_void_p()
        kinds, forms, ms = (ctypes.c_int * 256)(), (ctypes.c_int * 256)(), (ctypes.c_double * 256)()
        rp, ci = np.array(row_ptr, dtype=np.uint64), np.array(col_idx, dtype=np.uint32)
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            for bad in (c.p, c.n, 0):
                xb = c.up(xs[:cols - 1] + [bad])
                L.pgpu_timing_collect_ex(kinds, forms, ms, 256)
                assert L.pgpu_batch_ct_spmv_signed(c.pk._h, xb, rp.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p), wb,
                                                   4, 32, ctypes.byref(out)) == NOT_INVERTIBLE
                assert not out.value and b"unit" in L.pgpu_last_error()
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 256)
                seen = [kinds[i] for i in range(n)]
                assert KIND_INVERT in seen and KIND_SPMV not in seen, seen
                # the unsigned call never reads that column
                assert R.down(spmv(c, L.pgpu_batch_ct_spmv, xb, row_ptr, col_idx, R.up([abs(v) for v in wt], 1), 32)) == \
                    expect(xs, row_ptr, col_idx, [abs(v) for v in wt], c.nsq)
                assert R.down(spmv_s(c, c.up(xs), row_ptr, col_idx, wb, 32)) == want
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_refusals_are_host_side_and_launch_kinds(engine, knobs):
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(10)
    kinds, forms, ms = (ctypes.c_int * 128)(), (ctypes.c_int * 128)(), (ctypes.c_double * 128)()
    try:
        cols = 8
        xs = c.units(rng, cols)
        x = c.up(xs)
        xp = c.encrypt(list(range(1, 9)), rng)
        row_ptr, col_idx = csr(rng, [3, 0, 9, 2], cols)
        wt = rand_weights(rng, 14, 32)
        wb = up_w(c, wt, 32)
        other = engine.PublicKey(int(json.load(open(os.path.join(ROOT, "tests", "golden", "aggregate_refusals.json")))["other_n"]["2048"], 16), 2048)
        pair_other = R.op(L.pgpu_batch_ct_add, other._h, c.up(xs), c.up(xs))
        wide = R.up(xs, 2 * c.nw + 1)
        out = ctypes.c_void_p()
        k = c.pk._h

        def call(key, xb, rp, ci, wbatch, rows, e_bits):
            a = None if rp is None else np.array(rp, dtype=np.uint64)
            b = None if ci is None else np.array(ci, dtype=np.uint32)
            return L.pgpu_batch_ct_spmv_signed(key, xb, None if a is None else a.ctypes.data_as(ctypes.c_void_p),
                                               None if b is None else b.ctypes.data_as(ctypes.c_void_p), wbatch, rows, e_bits, ctypes.byref(out))
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 128)
            invalid = [
                ((None, x, row_ptr, col_idx, wb, 4, 32), b"null"), ((k, None, row_ptr, col_idx, wb, 4, 32), b"null"),
                ((k, x, None, col_idx, wb, 4, 32), b"null"), ((k, x, row_ptr, None, wb, 4, 32), b"null"),
                ((k, x, row_ptr, col_idx, None, 4, 32), b"null"),
                ((k, x, row_ptr, col_idx, wb, 0, 32), b"rows must be positive"),
                ((k, x, [1] + row_ptr[1:], col_idx, wb, 4, 32), b"row_ptr[0] must be 0"),
                ((k, x, [0, 3, 2, 12, 14], col_idx, wb, 4, 32), b"non-decreasing"),
                ((k, x, [0, 0, 0, 0, 0], col_idx, wb, 4, 32), b"no entries"),
                ((k, x, row_ptr[:4], col_idx, wb, 3, 32), b"Size mismatch"),
                ((k, x, row_ptr, [cols] + col_idx[1:], wb, 4, 32), b"column index"),
                ((k, x, row_ptr, col_idx, xp, 4, 32), b"plain uploaded batch"),
                ((k, x, row_ptr, col_idx, wb, 4, 0), b"e_bits"), ((k, x, row_ptr, col_idx, wb, 4, 65), b"e_bits"),
                ((k, wide, row_ptr, col_idx, wb, 4, 32), b"ciphertext width mismatch"),
                ((k, pair_other, row_ptr, col_idx, wb, 4, 32), b"different key")]
            for args, text in invalid:
                assert call(*args) == INVALID, args
                assert text in L.pgpu_last_error() and not out.value, (args, L.pgpu_last_error())
            assert L.pgpu_set_table_gather_policy(1) == 0
            try:
                assert call(k, x, row_ptr, col_idx, wb, 4, 32) == UNSUPPORTED
                err = L.pgpu_last_error()
                assert b"signed spmv" in err and b"masked" in err and b"plaintext column numbers" in err and not out.value
            finally:
                L.pgpu_set_table_gather_policy(0)
            p4, q4, _ = key_case(4096, False)
            pk4 = engine.PublicKey(p4 * q4, 4096)
            assert call(pk4._h, R.up([3, 5], 128), [0, 2], [0, 1], R.up([1, 2], 1), 1, 32) == UNSUPPORTED
            assert b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 128) == 0    # nothing was launched
            # the launch kinds of a call: the inversion's first, then table build, multi-exponentiation and fold levels
            knobs(None, 2)                                                 # the row of 9 entries: five chains, three fold levels
            y = spmv_s(c, x, row_ptr, col_idx, wb, 32)
            assert L.pgpu_synchronize() == 0
            n = L.pgpu_timing_collect_ex(kinds, forms, ms, 128)
            seen = [kinds[i] for i in range(n)]
            levels = ctypes.c_int()
            assert L.pgpu_ct_spmv_signed_plan(2048, 4, cols, 14, 9, 32, None, None, ctypes.byref(levels), None, None) == 0
            n_inv = ctypes.c_int()
            assert L.pgpu_ct_negate_plan(2048, cols, None, None, ctypes.byref(n_inv), None) == 0
            last = max(i for i in range(n) if seen[i] == KIND_INVERT)       # (the grand total's conversions lie between them)
            assert seen.count(KIND_INVERT) == n_inv.value and KIND_SPMV not in seen[:last], seen   # every column of x, referenced or not
            assert seen[last + 1:] == [KIND_SPMV] * (1 + levels.value), seen
            assert R.down(y) == expect(xs, row_ptr, col_idx, wt, c.nsq)
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_python_keyword(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(5)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    m = [rng.randrange(1 << 40) for _ in range(7)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    indptr, indices = [0, 3, 3, 5, 9], [0, 6, 2, 1, 1, 5, 4, 3, 0]
    wt = [-3, 7, -(1 << 40), 5, -5, 1, 0, -1, (1 << 40) - 1]
    y = pk.spmv(ct, indptr, indices, wt, signed=True)
    assert y == expect(ct, indptr, indices, wt, n * n)
    assert sk.decrypt(y) == [sum(wt[t] * m[indices[t]] for t in range(indptr[i], indptr[i + 1])) % n for i in range(4)]
    assert y[1] == 1 and y[2] == 1                                    # an empty row; weights 5 and -5 on one column
    assert pk.spmv(ct, indptr, indices, wt, e_bits=50, signed=True) == y
    with pytest.raises(RuntimeError, match="spmv error: negative weights have no encoding"):
        pk.spmv(ct, indptr, indices, wt)                              # signed=False: today's behaviour
    pos = [abs(v) for v in wt]
    assert pk.spmv(ct, indptr, indices, pos) == pk.spmv(ct, indptr, indices, pos, signed=True)
