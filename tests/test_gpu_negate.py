"""Ciphertext negation and subtraction on resident ciphertexts (pgpu_batch_ct_negate / pgpu_batch_ct_sub;
csrc/hensel_invert.hpp) on the GPU:
    negate   out[i] = x[i]^-1 mod n^2               sub   out[i] = a[i] * b[i]^-1 mod n^2
held bit-identical to Python's pow(c, -1, n^2) for the 1024-, 2048- and 3072-bit key classes: one chain, a short last
chain, counts that are no multiple of the chains of a wavefront, more than one level; forced chunks that reach three and
four levels, both forms of a 2048-bit key, key widths off the standard classes, edge ciphertexts, inputs in every form a
resident ciphertext batch can have, the round trips through CRT decrypt (the sibling histogram, signed weights composed
from two matvecs), the agreement with the exponentiation by n - 1, the broadcast b, two lanes at once, the timing record
and the refusals -- the one that follows launches among them.  The reference has no such operation: its route to Enc(-m)
is CipherText::operator*(PlainText) with n - 1 (ipcl/ciphertext.cpp:83-107)."""
import ctypes
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from test_gpu_pair_rows import Res, key_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [1024, 2048, 3072]
COUNTS = [1, 2, 3, 7, 8, 9, 17, 65, 300]
KIND_INVERT, KIND_MODMUL, FORM_SEQ = 14, 2, 2        # PGPU_KERNEL_INVERT, PGPU_KERNEL_MODMUL, PGPU_FORM_SEQ (include/pgpu.h)
NOT_INVERTIBLE = -6                                  # PGPU_ERR_NOT_INVERTIBLE
SEGMENT_NONE = 0xFFFFFFFF


class Case:
    """a key, and helpers that keep everything resident"""

    def __init__(self, engine, bits):
        self.bits = bits
        self.p, self.q, self.hs = key_case(bits, True)
        self.n = self.p * self.q
        self.nsq = self.n * self.n
        self.nw = bits // 64
        self.pk, self.sk = engine.PublicKey(self.n, bits, hs=self.hs), engine.PrivateKey(self.p, self.q)
        self.R = Res()
        self.L = self.R.L

    def encrypt(self, m, rng):
        rw = self.bits // 128
        r = [rng.getrandbits(64 * rw) for _ in m]
        return self.R.op(self.L.pgpu_batch_encrypt, self.pk._h, self.R.up(m, self.nw), self.R.up(r, rw), 64 * rw)

    def up(self, xs):
        return self.R.up(xs, 2 * self.nw)

    def negate(self, x):
        return self.R.op(self.L.pgpu_batch_ct_negate, self.pk._h, x)

    def sub(self, a, b):
        return self.R.op(self.L.pgpu_batch_ct_sub, self.pk._h, a, b)

    def decrypt(self, h):
        return self.R.down(self.R.op(self.L.pgpu_batch_decrypt_crt, self.sk._h, h))

    def inv(self, xs):
        return [pow(v, -1, self.nsq) for v in xs]

    def units(self, rng, count):
        out = []
        while len(out) < count:
            v = rng.randrange(1, self.nsq)
            if v % self.p and v % self.q:
                out.append(v)
        return out

    def plan(self, count):
        chunk, levels, launches, products = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert self.L.pgpu_ct_negate_plan(self.bits, count, ctypes.byref(chunk), ctypes.byref(levels), ctypes.byref(launches),
                                          ctypes.byref(products)) == 0
        return chunk.value, levels.value, launches.value, products.value


@pytest.fixture
def knobs(monkeypatch):
    for name in ("PGPU_INVERT_CHUNK", "PGPU_INVERT_WIDE", "PGPU_SEGSCAN_CHUNK", "PGPU_SEGSUM_CHUNK"):
        monkeypatch.delenv(name, raising=False)

    def force(chunk=None, wide=None):
        for name, v in (("PGPU_INVERT_CHUNK", chunk), ("PGPU_INVERT_WIDE", wide)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


def model_levels(chunk, count):
    """levels of a plan whose every level has the same chunk: forced ones, and the pairs of every count that cannot fill the chip"""
    levels = 1
    while count > chunk:
        count = -(-count // chunk)
        levels += 1
    return levels


@pytest.mark.parametrize("bits", BITS)
def test_negate_and_sub_are_exact_at_every_count(engine, knobs, bits):
    """uploaded plain ciphertext words; the chunk the policy picks for counts that cannot fill the chip: pairs, up to nine levels"""
    c = Case(engine, bits)
    rng = random.Random(bits)
    L = c.L
    try:
        pool_a, pool_b = c.units(rng, 300), c.units(rng, 300)
        inv_b = c.inv(pool_b)
        for count in COUNTS:
            xs, ys = pool_a[:count], pool_b[:count]
            a, b = c.up(xs), c.up(ys)
            assert c.plan(count) == (2, model_levels(2, count), 1 if count == 1 else 2 * model_levels(2, count), 3 * (count - 1))
            y = c.negate(b)
            assert L.pgpu_batch_count(y) == count and L.pgpu_batch_row_limbs(y) > 0 and L.pgpu_batch_lane(y) == L.pgpu_batch_lane(b)
            assert c.R.down(y) == inv_b[:count], count
            d = c.sub(a, b)
            assert L.pgpu_batch_count(d) == count and L.pgpu_batch_row_limbs(d) > 0 and L.pgpu_batch_lane(d) == L.pgpu_batch_lane(a)
            assert c.R.down(d) == [u * v % c.nsq for u, v in zip(xs, inv_b)], count
            assert c.R.down(a) == xs and c.R.down(b) == ys      # the operands are left as they were
            c.R.close()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_forced_chunks_reach_three_and_more_levels(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    try:
        pool_a, pool_b = c.units(rng, 65), c.units(rng, 65)
        inv_b = c.inv(pool_b)
        for chunk, counts in ((2, (2, 3, 5, 9)), (3, (3, 4, 10, 28)), (8, (8, 9, 65))):
            knobs(chunk)
            for count in counts:
                got = c.plan(count)
                levels = model_levels(chunk, count)
                assert got == (chunk, levels, 2 * levels, 3 * (count - 1))
                a, b = c.up(pool_a[:count]), c.up(pool_b[:count])
                assert c.R.down(c.negate(b)) == inv_b[:count], (chunk, count)
                assert c.R.down(c.sub(a, b)) == [u * v % c.nsq for u, v in zip(pool_a, inv_b[:count])], (chunk, count)
            c.R.close()
        knobs(2)
        assert c.plan(9)[1] == 4 and c.plan(5)[1] == 3 and c.plan(3)[1] == 2
        knobs(3)
        assert c.plan(28)[1] == 4 and c.plan(9)[1] == 2 and c.plan(10)[1] == 3
    finally:
        c.R.close()


def test_both_forms_of_a_2048_bit_key(engine, knobs):
    """PGPU_INVERT_WIDE forces (4,18) or (8,9) for every level: the same canonical values"""
    c = Case(engine, 2048)
    rng = random.Random(5)
    try:
        xs, ys = c.units(rng, 65), c.units(rng, 65)
        want_n = c.inv(ys)
        want_s = [u * v % c.nsq for u, v in zip(xs, want_n)]
        a, b = c.up(xs), c.up(ys)
        for wide in (0, 1, None):
            for chunk in (None, 3):
                knobs(chunk, wide)
                assert c.R.down(c.negate(b)) == want_n, (wide, chunk)
                assert c.R.down(c.sub(a, b)) == want_s, (wide, chunk)
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", [1536, 2051, 2560])
def test_key_widths_off_the_standard_classes(engine, knobs, bits):
    """1536 and 2051: (4,18) with the wide (8,9) beside it; 2560: (8,14)"""
    from test_gpu_key_widths import Key
    K = Key(engine, bits)
    rng = random.Random(bits)
    L, R = K.L, K.R
    try:
        x, m = K.fresh(rng, 19)
        y, m2 = K.fresh(rng, 19)
        xs, ys = R.down(x), R.down(y)
        for wide in ((0, 1) if bits <= 2051 else (None,)):
            knobs(3, wide)
            neg = R.op(L.pgpu_batch_ct_negate, K.pk._h, x)
            assert R.down(neg) == [pow(v, -1, K.nsq) for v in xs]
            d = R.op(L.pgpu_batch_ct_sub, K.pk._h, x, y)
            assert R.down(d) == [u * pow(v, -1, K.nsq) % K.nsq for u, v in zip(xs, ys)]
        assert K.decrypt(neg) == [(-v) % K.n for v in m]
        assert K.decrypt(d) == [(u - v) % K.n for u, v in zip(m, m2)]
    finally:
        K.close()


@pytest.mark.parametrize("bits", BITS)
def test_edge_values(engine, knobs, bits):
    """1, n^2 - 1, n + 1 and (n + 1)^(n - 1) in runs, at the start and the end of a chain"""
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    try:
        edge = [1, c.nsq - 1, c.n + 1, (1 + c.n * (c.n - 1)) % c.nsq]     # (n + 1)^k == 1 + k n modulo n^2
        xs = edge + c.units(rng, 4) + edge[::-1] + [1, 1, 1, 1] + [c.nsq - 1] * 4 + c.units(rng, 1) + [c.n + 1]
        ys = c.units(rng, len(xs))
        want = c.inv(xs)
        x, y = c.up(xs), c.up(ys)
        for chunk in (None, 3, 8):
            knobs(chunk)
            assert c.R.down(c.negate(x)) == want, chunk
            assert c.R.down(c.sub(y, x)) == [u * v % c.nsq for u, v in zip(ys, want)], chunk
            assert c.R.down(c.sub(x, y)) == [u * pow(v, -1, c.nsq) % c.nsq for u, v in zip(xs, ys)], chunk
        ones = c.up([1] * 10)
        assert c.R.down(c.negate(ones)) == [1] * 10 and c.R.down(c.sub(ones, ones)) == [1] * 10
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_inputs_in_every_form_and_round_trips(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    try:
        count = 33
        ma, mb = [rng.randrange(c.n) for _ in range(count)], [rng.randrange(c.n) for _ in range(count)]
        a, b = c.encrypt(ma, rng), c.encrypt(mb, rng)             # resident DJN encrypt: pair rows
        xa, xb = R.down(a), R.down(b)
        want = c.inv(xb)
        y = c.negate(b)
        assert R.down(y) == want
        assert R.down(c.negate(c.up(xb))) == want                # uploaded plain ciphertext words
        assert R.down(c.sub(c.up(xa), b)) == R.down(c.sub(a, c.up(xb))) == [u * v % c.nsq for u, v in zip(xa, want)]
        # the output of a previous negate: negate(negate(x)) == x bit for bit, across the level boundaries too
        knobs(4)
        assert R.down(c.negate(y)) == xb
        knobs(None)
        # round trips through CRT decrypt
        assert c.decrypt(y) == [(-v) % c.n for v in mb]
        assert c.decrypt(c.sub(a, b)) == [(u - v) % c.n for u, v in zip(ma, mb)]
        assert c.decrypt(c.sub(a, a)) == [0] * count and R.down(c.sub(a, a)) == [1] * count
        # the same decryption as the route of the parent commit: CT x PT by the one-element exponent n - 1
        e = R.up([c.n - 1], c.nw)
        via_mul = R.op(L.pgpu_batch_ct_mul, c.pk._h, b, e, bits)
        assert c.decrypt(via_mul) == c.decrypt(y)
        # the outputs of segment_sum and segment_scan
        n_segments = 5
        ids = [rng.randrange(n_segments) for _ in range(count)]
        arr = np.array(ids, dtype=np.uint32)
        h = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, a, arr.ctypes.data_as(ctypes.c_void_p), 1, n_segments)
        hs = R.down(h)
        assert R.down(c.negate(h)) == c.inv(hs)
        s = R.op(L.pgpu_batch_ct_segment_scan, c.pk._h, b, 11, 0)
        ss = R.down(s)
        assert R.down(c.negate(s)) == c.inv(ss)
        assert R.down(c.sub(s, b)) == [u * v % c.nsq for u, v in zip(ss, want)]
        # sibling = parent - child: the histogram of the complement, without building it
        child = [rng.randrange(2) for _ in range(count)]
        ids_child = np.array([i if f else SEGMENT_NONE for i, f in zip(ids, child)], dtype=np.uint32)
        ids_rest = np.array([SEGMENT_NONE if f else i for i, f in zip(ids, child)], dtype=np.uint32)
        hc = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, a, ids_child.ctypes.data_as(ctypes.c_void_p), 1, n_segments)
        hr = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, a, ids_rest.ctypes.data_as(ctypes.c_void_p), 1, n_segments)
        sibling = c.decrypt(c.sub(h, hc))
        assert sibling == c.decrypt(hr)
        assert sibling == [sum(m for m, i, f in zip(ma, ids, child) if i == s_ and not f) % c.n for s_ in range(n_segments)]
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_signed_weights_composed_from_two_matvecs(engine, knobs, bits):
    """sub(matvec(x, W+), matvec(x, W-)) decrypts to the signed W m mod n: 32-bit exponents instead of key-width ones"""
    c = Case(engine, bits)
    rng = random.Random(bits + 4)
    L, R = c.L, c.R
    try:
        rows, cols = 3, 5
        m = [rng.randrange(c.n) for _ in range(cols)]
        W = [[rng.randrange(-(1 << 31), 1 << 31) for _ in range(cols)] for _ in range(rows)]
        W[0][0], W[1][1], W[2][2] = 0, -1, (1 << 31) - 1
        assert any(v < 0 for r in W for v in r) and any(v > 0 for r in W for v in r)
        x = c.encrypt(m, rng)
        wp = R.up([max(v, 0) for r in W for v in r], 1)
        wn = R.up([max(-v, 0) for r in W for v in r], 1)
        pos = R.op(L.pgpu_batch_ct_matvec, c.pk._h, x, wp, rows, 32)
        neg = R.op(L.pgpu_batch_ct_matvec, c.pk._h, x, wn, rows, 32)
        assert c.decrypt(c.sub(pos, neg)) == [sum(w * v for w, v in zip(r, m)) % c.n for r in W]
    finally:
        R.close()


def test_broadcast_b(engine, knobs):
    c = Case(engine, 2048)
    rng = random.Random(6)
    R = c.R
    try:
        for count in (2, 9, 65):
            xs, (y,) = c.units(rng, count), c.units(rng, 1)
            yi = pow(y, -1, c.nsq)
            a, b = c.up(xs), c.up([y])
            d = c.sub(a, b)
            assert c.L.pgpu_batch_count(d) == count
            assert R.down(d) == [u * yi % c.nsq for u in xs]
            assert R.down(b) == [y] and R.down(a) == xs
        m = [rng.randrange(c.n) for _ in range(7)]
        ea, eb = c.encrypt(m, rng), c.encrypt([12345], rng)
        assert c.decrypt(c.sub(ea, eb)) == [(v - 12345) % c.n for v in m]
    finally:
        R.close()


def test_two_lanes_at_once(engine, knobs):
    """two threads on different batch lanes, each with its own inputs; the second operand of one sub lives on the other lane"""
    c = Case(engine, 2048)
    L = c.L
    results, errors = {}, []
    rng = random.Random(8)
    shared_vals = c.units(rng, 40)
    shared = c.up(shared_vals)                         # lane of the main thread: ordered in by events

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            r = random.Random(700 + lane)
            count = 40
            xs = c.units(r, count)
            x = R.up(xs, 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            y = R.op(L.pgpu_batch_ct_negate, c.pk._h, x)
            d = R.op(L.pgpu_batch_ct_sub, c.pk._h, x, shared)
            assert L.pgpu_batch_lane(y) == lane and L.pgpu_batch_lane(d) == lane
            results[lane] = (R.down(y), R.down(d), xs)
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    try:
        ts = [threading.Thread(target=worker, args=(lane,)) for lane in (1, 2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert len(results) == 2
        inv_shared = c.inv(shared_vals)
        for neg, dif, xs in results.values():
            assert neg == c.inv(xs)
            assert dif == [u * v % c.nsq for u, v in zip(xs, inv_shared)]
    finally:
        c.R.close()


def test_launches_carry_the_invert_kind(engine, knobs):
    c = Case(engine, 2048)
    rng = random.Random(11)
    L, R = c.L, c.R
    try:
        knobs(4)
        x = c.encrypt([rng.randrange(c.n) for _ in range(21)], rng)        # pair rows already: no conversion of the operand
        a = c.encrypt([rng.randrange(c.n) for _ in range(21)], rng)
        xs, as_ = R.down(x), R.down(a)
        chunk, levels, launches, products = c.plan(21)                     # chunk 4: 21 -> 6 totals -> 2 totals: three levels
        assert (chunk, levels, launches, products) == (4, 3, 6, 60)
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_set_timing(1) == 0
        try:
            for call, want in ((lambda: c.negate(x), c.inv(xs)),
                               (lambda: c.sub(a, x), [u * v % c.nsq for u, v in zip(as_, c.inv(xs))])):
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)             # drop what earlier calls left
                y = call()
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)         # (before the download, which may launch a conversion)
                assert R.down(y) == want
                mine = [i for i in range(n) if kinds[i] == KIND_INVERT]
                assert len(mine) == launches                               # a forward pass and a walk back per level
                assert all(forms[i] == FORM_SEQ and ms[i] > 0 for i in mine)
                # beside them only the grand total on its way down and its inverse on its way up: two row conversions
                assert [kinds[i] for i in range(n) if i not in mine] == [KIND_MODMUL] * 2
            knobs(None)
            one = c.encrypt([7], rng)
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
            y = c.negate(one)
            assert L.pgpu_synchronize() == 0
            n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
            assert c.plan(1) == (2, 1, 1, 0)
            assert [kinds[i] for i in range(n)].count(KIND_INVERT) == 1    # count == 1: one walk back, no forward pass
            assert c.decrypt(y) == [c.n - 7]
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_refusals_are_host_side(engine, knobs):
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(10)
    try:
        xs = c.units(rng, 6)
        x, x4 = c.up(xs), c.up(xs[:4])
        out = ctypes.c_void_p()

        def neg(key, xb):
            return L.pgpu_batch_ct_negate(key, xb, ctypes.byref(out))

        def sub(key, ab, bb):
            return L.pgpu_batch_ct_sub(key, ab, bb, ctypes.byref(out))
        assert neg(None, x) == -1 and neg(c.pk._h, None) == -1 and L.pgpu_batch_ct_negate(c.pk._h, x, None) == -1
        assert sub(None, x, x) == -1 and sub(c.pk._h, None, x) == -1 and sub(c.pk._h, x, None) == -1
        assert L.pgpu_batch_ct_sub(c.pk._h, x, x, None) == -1
        assert sub(c.pk._h, x, x4) == -1 and b"Size mismatch" in L.pgpu_last_error()   # count(b) neither count(a) nor 1
        assert sub(c.pk._h, x4, x) == -1
        narrow = R.up([3, 5, 7, 9, 11, 13], c.nw)
        assert neg(c.pk._h, narrow) == -1 and b"width" in L.pgpu_last_error()
        assert sub(c.pk._h, x, narrow) == -1 and sub(c.pk._h, narrow, x) == -1
        # a batch of another key: pair rows of a 1024-bit key, and words of the wrong width
        c1 = Case(engine, 1024)
        try:
            x1 = c1.encrypt([1, 2, 3, 4, 5, 6], rng)
            assert neg(c.pk._h, x1) == -1 and sub(c.pk._h, x, x1) == -1 and sub(c.pk._h, x1, x) == -1
            p3, q3, hs3 = key_case(3072, True)
            pk3 = engine.PublicKey(p3 * q3, 3072, hs=hs3)
            assert neg(pk3._h, x) == -1 and sub(pk3._h, x, x) == -1
        finally:
            c1.R.close()
        assert not out.value                                   # (stale handles: test_stale_handles_are_refused, own process)
        # the masked table-gather policy: refused, and the text says why
        assert L.pgpu_set_table_gather_policy(1) == 0
        try:
            assert neg(c.pk._h, x) == -3 and b"masked" in L.pgpu_last_error() and not out.value
            assert sub(c.pk._h, x, x) == -3 and b"masked" in L.pgpu_last_error() and not out.value
        finally:
            L.pgpu_set_table_gather_policy(0)
        assert R.down(c.negate(x)) == c.inv(xs)
        # a key class without pair rows
        p4, q4, _ = key_case(4096, False)
        pk4 = engine.PublicKey(p4 * q4, 4096)
        w4 = R.up([3, 5], 128)
        assert neg(pk4._h, w4) == -3 and b"pair" in L.pgpu_last_error() and not out.value
        assert sub(pk4._h, w4, w4) == -3 and not out.value
        chunk, levels, launches, products = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        args = (ctypes.byref(chunk), ctypes.byref(levels), ctypes.byref(launches), ctypes.byref(products))
        assert L.pgpu_ct_negate_plan(4096, 10, *args) == -3
        assert L.pgpu_ct_negate_plan(2048, 0, *args) == -1 and L.pgpu_ct_negate_plan(0, 10, *args) == -1
        knobs(2)                                                                   # more chains than a descriptor addresses
        assert L.pgpu_ct_negate_plan(2048, 1 << 33, *args) == -1 and b"chains" in L.pgpu_last_error()
        assert L.pgpu_ct_negate_plan(2048, 9, None, None, None, None) == 0
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_a_non_unit_is_refused_after_the_forward_pass(engine, knobs, bits):
    """0, p and n are no ciphertexts: PGPU_ERR_NOT_INVERTIBLE, *out untouched, and the lane stays usable"""
    c = Case(engine, bits)
    rng = random.Random(bits + 9)
    L, R = c.L, c.R
    try:
        good = c.units(rng, 20)
        ok = c.up(good)
        want = c.inv(good)
        out = ctypes.c_void_p()
        for bad in (0, c.p, c.n):
            for at in (0, 13, 19):
                for chunk in (None, 3):
                    knobs(chunk)
                    xs = list(good)
                    xs[at] = bad
                    x = c.up(xs)
                    assert L.pgpu_batch_ct_negate(c.pk._h, x, ctypes.byref(out)) == NOT_INVERTIBLE and not out.value
                    assert b"unit" in L.pgpu_last_error()
                    assert L.pgpu_batch_ct_sub(c.pk._h, ok, x, ctypes.byref(out)) == NOT_INVERTIBLE and not out.value
                    assert R.down(c.negate(ok)) == want            # a correct negate on the same lane straight after
                    assert R.down(c.sub(x, ok)) == [u * v % c.nsq for u, v in zip(xs, want)]   # (a non-unit may be subtracted FROM)
            R.close()
            ok = c.up(good)
        one = c.up([c.p])
        assert L.pgpu_batch_ct_negate(c.pk._h, one, ctypes.byref(out)) == NOT_INVERTIBLE and not out.value
        assert L.pgpu_batch_ct_sub(c.pk._h, ok, one, ctypes.byref(out)) == NOT_INVERTIBLE and not out.value   # the broadcast b
        assert R.down(c.negate(ok)) == want
    finally:
        R.close()


_NO_PAIR_ROWS = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
pk = pa.PublicKey(p * q, 2048, hs=hs)
R = Res()
x = R.up([3, 5, 7, 9], 64)
out = ctypes.c_void_p()
rc = R.L.pgpu_batch_ct_negate(pk._h, x, ctypes.byref(out))
print("rc", rc, R.L.pgpu_last_error().decode())
rc2 = R.L.pgpu_batch_ct_sub(pk._h, x, x, ctypes.byref(out))
print("rc", rc2, R.L.pgpu_last_error().decode())
R.close()
sys.exit(0 if rc == -3 and rc2 == -3 and not out.value else 1)
"""


_STALE = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
nsq = (p * q) ** 2
R = Res()
L = R.L
old_key = pa.PublicKey(p * q, 2048, hs=hs)
old_x = R.up([3, 5, 7, 9], 64)
L.pgpu_shutdown()                      # the pool the key and the batch were created under is gone
pa.initialize()
new_key = pa.PublicKey(p * q, 2048, hs=hs)
new_x = R.up([3, 5, 7, 9], 64)
out = ctypes.c_void_p()
ok = True
for key, x in ((old_key, new_x), (new_key, old_x), (old_key, old_x)):
    rc = L.pgpu_batch_ct_negate(key._h, x, ctypes.byref(out))
    print("rc", rc, L.pgpu_last_error().decode())
    ok = ok and rc == -1 and b"shut down" in L.pgpu_last_error() and not out.value
for key, a, b in ((old_key, new_x, new_x), (new_key, old_x, new_x), (new_key, new_x, old_x)):
    rc = L.pgpu_batch_ct_sub(key._h, a, b, ctypes.byref(out))
    print("rc", rc, L.pgpu_last_error().decode())
    ok = ok and rc == -1 and b"shut down" in L.pgpu_last_error() and not out.value
rc = L.pgpu_batch_ct_negate(new_key._h, new_x, ctypes.byref(out))
ok = ok and rc == 0 and bool(out.value)
if out.value:
    got = R.down(out)
    L.pgpu_batch_destroy(out)
    ok = ok and got == [pow(v, -1, nsq) for v in (3, 5, 7, 9)]
    print("negate", ok)
L.pgpu_batch_destroy(new_x)
sys.exit(0 if ok else 1)
"""


def test_stale_handles_are_refused(engine):
    """a key or a batch created under a device pool that has been shut down: PGPU_ERR_INVALID_PARAM, *out untouched (own
    process: the pool of the test session stays up)"""
    r = subprocess.run([sys.executable, "-c", _STALE, ROOT], capture_output=True, text=True, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


@pytest.mark.parametrize("switch", ["PGPU_PAIR_ROWS", "PGPU_HENSEL"])
def test_refused_without_pair_rows(engine, switch):
    """PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 keep resident ciphertexts as Montgomery-form words: no pair form,
    PGPU_ERR_UNSUPPORTED (own process: the switches are read once)"""
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, "-c", _NO_PAIR_ROWS, ROOT], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


def test_python_negate_and_sub(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(4)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    ma, mb = [rng.randrange(1 << 40) for _ in range(12)], [rng.randrange(1 << 40) for _ in range(12)]
    ca, cb = pk.encrypt(ma, [rng.getrandbits(1024) for _ in ma]), pk.encrypt(mb, [rng.getrandbits(1024) for _ in mb])
    neg = pk.negate(ca)
    assert neg == [pow(v, -1, n * n) for v in ca]
    assert sk.decrypt(neg) == [n - v for v in ma]
    assert sk.decrypt(pk.sub(ca, cb)) == [(u - v) % n for u, v in zip(ma, mb)]
    assert sk.decrypt(pk.sub(ca, cb[:1])) == [(u - mb[0]) % n for u in ma]
    with pytest.raises(RuntimeError):
        pk.negate([])
    with pytest.raises(RuntimeError):
        pk.sub(ca, cb[:5])
    with pytest.raises(RuntimeError):
        pk.sub([], [])
    with pytest.raises(RuntimeError):
        pk.negate(ca[:3] + [p] + ca[3:])                                  # not a unit modulo n: no inverse
