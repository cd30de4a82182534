"""The encrypted weighted sum of K resident ciphertext batches (pgpu_batch_ct_weighted_sum; csrc/hensel_wsum.hpp) on the GPU:
    out[i] = prod_k xs[k][i]^(a_k) mod n^2
held bit-identical to Python's pow for the 1024-, 2048- and 3072-bit key classes, the 2048-bit class in both of its forms:
counts that are ragged for 8 / 16 / 32 groups per wavefront and reach a second workgroup; K from 1 to 17 with weights 0,
1, 2^32 - 1, a lone top bit, 65 and 100 bits; no weights at all; every weight zero; the full-width weight n - 1; operands
in every form within one call; forced slices against the default plan; the round trip through CRT decrypt and the
agreement with the composed CT x PT + CT + CT route; key widths off the standard classes; the timing record; the refusals;
two lanes at once.  Everything is exact: there are no tolerances.  In the reference such a sum is composed from
CipherText::operator* (ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72) term by term."""
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
KIND_WSUM, FORM_SEQ = 10, 2           # PGPU_KERNEL_WSUM, PGPU_FORM_SEQ (include/pgpu.h)
INVALID, UNSUPPORTED = -1, -3
FORMS = [(1024, None), (2048, 0), (2048, 1), (3072, None)]      # (bits, PGPU_WSUM_WIDE)
KS = (1, 2, 3, 5, 17)


def term_weights(rng):
    """one weight per term position, 17 of them; a call over K terms uses the first K"""
    w = [(1 << 32) - 1, 0, 1, 1 << 63, rng.getrandbits(64) | (1 << 64), rng.getrandbits(99) | (1 << 99), rng.getrandbits(32)]
    w += [0, 0, 5, rng.getrandbits(32), 1, rng.getrandbits(13), 1 << 31, rng.getrandbits(32), 0, rng.getrandbits(32) | 1]
    assert len(w) == 17
    return w


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

    def encrypt(self, m, rng, R=None):
        R = R or self.R
        rw = self.bits // 128
        r = [rng.getrandbits(64 * rw) for _ in m]
        return R.op(self.L.pgpu_batch_encrypt, self.pk._h, R.up(m, self.nw), R.up(r, rw), 64 * rw)


def wsum(L, R, key, hs, weights, words=None):
    """one pgpu_batch_ct_weighted_sum call; weights: ints, or None"""
    arr = (ctypes.c_void_p * len(hs))(*[h.value for h in hs])
    if weights is None:
        return R.op(L.pgpu_batch_ct_weighted_sum, key, arr, len(hs), None, 0)
    ww = words or max(1, (max(v.bit_length() for v in weights) + 63) // 64)
    wa = R.i2l(weights, ww)
    y = R.op(L.pgpu_batch_ct_weighted_sum, key, arr, len(hs), wa.ctypes.data_as(ctypes.c_void_p), ww)
    wa[:] = 0xFFFFFFFFFFFFFFFF                                     # the weights are consumed before the call returns
    return y


def expect(xs, weights, nsq):
    out = []
    for i in range(len(xs[0])):
        acc = 1
        for k, x in enumerate(xs):
            a = 1 if weights is None else weights[k]
            if a:
                acc = acc * pow(x[i], a, nsq) % nsq
        out.append(acc)
    return out


@pytest.fixture
def knobs(monkeypatch):
    names = ("PGPU_WSUM_SLICES", "PGPU_WSUM_WIDE")
    for name in names:
        monkeypatch.delenv(name, raising=False)

    def force(slices=None, wide=None):
        for name, v in zip(names, (slices, wide)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


@pytest.mark.parametrize("count", [1, 17, 33, 130])
@pytest.mark.parametrize("bits,wide", FORMS)
def test_every_shape_is_exact(engine, knobs, bits, wide, count):
    """17 resident batches of `count` elements; every K of KS takes the first K of them with the first K weights, under
    the default plan (K = 17 at these counts: 4 slices and a fold); then no weights, every weight zero, and the copy"""
    c = Case(engine, bits)
    rng = random.Random(bits * 1000 + count)
    L, R = c.L, c.R
    knobs(None, wide)
    try:
        hs = [c.encrypt([rng.randrange(c.n) for _ in range(count)], rng) for _ in range(17)]     # resident DJN encrypt: pair rows
        xs = [R.down(h) for h in hs]
        w = term_weights(rng)
        powers = [[pow(v, a, c.nsq) if a else 1 for v in x] for x, a in zip(xs, w)]              # once, shared by every K
        for K in KS:
            want = [1] * count
            for k in range(K):
                want = [u * v % c.nsq for u, v in zip(want, powers[k])]
            y = wsum(L, R, c.pk._h, hs[:K], w[:K])
            assert L.pgpu_batch_count(y) == count and L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(hs[0]) > 0
            assert L.pgpu_batch_lane(y) == L.pgpu_batch_lane(hs[0])
            assert R.down(y) == want, K
        for K in (1, 2, 17):
            assert R.down(wsum(L, R, c.pk._h, hs[:K], None)) == expect(xs[:K], None, c.nsq), K   # weights == NULL: the plain sum
            assert R.down(wsum(L, R, c.pk._h, hs[:K], [0] * K)) == [1] * count, K                # every weight zero: the ciphertext 1
        assert R.down(wsum(L, R, c.pk._h, hs[:1], [1])) == xs[0]                                  # a copy
        assert [R.down(h) for h in hs] == xs                                                      # the inputs are unchanged
    finally:
        R.close()


@pytest.mark.parametrize("bits,wide", FORMS)
def test_full_width_weight(engine, knobs, bits, wide):
    """a mod n for a = -1: the longest squaring run there is, about 2 * bits serial products"""
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    L, R = c.L, c.R
    knobs(None, wide)
    try:
        hs = [c.encrypt([rng.randrange(c.n) for _ in range(3)], rng) for _ in range(2)]
        xs = [R.down(h) for h in hs]
        w = [c.n - 1, rng.randrange(c.n) | 1]
        y = wsum(L, R, c.pk._h, hs, w)
        assert R.down(y) == expect(xs, w, c.nsq)
    finally:
        R.close()


@pytest.mark.parametrize("bits,wide", FORMS)
def test_operands_in_every_form_in_one_call(engine, knobs, bits, wide):
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    L, R = c.L, c.R
    knobs(None, wide)
    try:
        count = 5
        a = c.encrypt([rng.randrange(c.n) for _ in range(count)], rng)          # resident DJN encrypt output: pair rows
        b_vals = [rng.randrange(1, c.nsq) for _ in range(count)]
        b = R.up(b_vals, 2 * c.nw)                                               # uploaded plain words
        s = R.op(L.pgpu_batch_ct_add, c.pk._h, a, b)                             # a CT + CT result
        t = R.op(L.pgpu_batch_ct_mul, c.pk._h, a, R.up([rng.getrandbits(20)], 1), 20)   # a CT x PT result
        edge_vals = [1, c.n + 1, c.nsq - 1, 1, c.nsq - 1]
        e = R.up(edge_vals, 2 * c.nw)                                            # the edge ciphertexts
        hs = [a, b, s, t, a, e, b]                                               # (a and b twice: once per appearance)
        xs = [R.down(h) for h in hs]
        for w in ([rng.getrandbits(32) | 1 for _ in hs], [3, 0, 1, 1 << 40, 7, (1 << 32) - 1, 2], None):
            want = expect(xs, w, c.nsq)
            for slices in (1, 3):
                knobs(slices, wide)
                assert R.down(wsum(L, R, c.pk._h, hs, w)) == want, (w, slices)
        assert [R.down(h) for h in hs] == xs
        assert R.down(b) == b_vals and R.down(e) == edge_vals
    finally:
        R.close()


@pytest.mark.parametrize("bits,wide", FORMS)
def test_slices_give_identical_bits(engine, knobs, bits, wide):
    """K = 17 over 33 elements: slices forced to 1, 2, 3 and K, and the default plan (4 slices here, by the plan query),
    give the same download; so do slices that are dropped because their weights are zero"""
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    try:
        count, K = 33, 17
        hs = [R.up([rng.randrange(1, c.nsq) for _ in range(count)], 2 * c.nw) for _ in range(K)]
        xs = [R.down(h) for h in hs]
        for w in ([rng.getrandbits(32) for _ in range(K)], [0] * 6 + [rng.getrandbits(17) for _ in range(5)] + [0] * 6, None):
            want = expect(xs, w, c.nsq)
            for slices in (1, 2, 3, K, None):
                knobs(slices, wide)
                assert R.down(wsum(L, R, c.pk._h, hs, w)) == want, slices
        knobs(None, wide)
        sl = ctypes.c_int()
        wa = R.i2l([1] * K, 1)
        assert L.pgpu_ct_weighted_sum_plan(bits, count, K, wa.ctypes.data_as(ctypes.c_void_p), 1, None, None, ctypes.byref(sl),
                                           None, None) == 0
        assert sl.value == 4                                                     # the default plan at a small count: S > 1
    finally:
        R.close()


@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_round_trip_and_composed_route(engine, knobs, bits):
    """CRT decrypt of the result is sum_k a_k m_k mod n; the composed route -- K CT x PT calls with a one-element exponent,
    K - 1 CT + CT calls -- downloads the same bits"""
    c = Case(engine, bits)
    rng = random.Random(bits + 4)
    L, R = c.L, c.R
    try:
        count, K = 19, 6
        ms = [[rng.randrange(c.n) for _ in range(count)] for _ in range(K)]
        hs = [c.encrypt(m, rng) for m in ms]
        w = [rng.getrandbits(32) for _ in range(K - 1)] + [c.n - 2]              # (-2 mod n among them)
        y = wsum(L, R, c.pk._h, hs, w)
        plain = [sum(a * m[i] for a, m in zip(w, ms)) % c.n for i in range(count)]
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, y)) == plain
        acc = None
        for h, a in zip(hs, w):
            ew = (a.bit_length() + 63) // 64
            term = R.op(L.pgpu_batch_ct_mul, c.pk._h, h, R.up([a], ew), 64 * ew)
            acc = term if acc is None else R.op(L.pgpu_batch_ct_add, c.pk._h, acc, term)
        assert R.down(y) == R.down(acc)
        # the result feeds CT + CT
        s = R.op(L.pgpu_batch_ct_add, c.pk._h, y, y)
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, s)) == [2 * v % c.n for v in plain]
    finally:
        R.close()


@pytest.mark.parametrize("count", [1, 37])
@pytest.mark.parametrize("bits", [1065, 1124, 2037, 3211])
def test_key_widths_off_the_standard_classes(engine, knobs, bits, count):
    from test_gpu_key_widths import Key
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + count)
    try:
        pairs = [K.fresh(rng, count) for _ in range(3)]
        hs = [x for x, _ in pairs] + [R.up([rng.randrange(1, K.nsq) for _ in range(count)], 2 * K.nw)]
        xs = [R.down(h) for h in hs]
        w = [rng.getrandbits(32), K.n - 1 if count == 1 else rng.getrandbits(100), 1, rng.getrandbits(65)]     # (-1 mod n once per width)
        want = expect(xs, w, K.nsq)
        for slices in (None, 2):
            knobs(slices)
            y = wsum(L, R, K.pk._h, hs, w)
            assert L.pgpu_batch_count(y) == count and L.pgpu_batch_row_limbs(y) == 2 * K.l2
            assert R.down(y) == want, slices
        y = wsum(L, R, K.pk._h, hs[:3], w[:3])
        assert K.decrypt(y) == [sum(a * m[i] for a, (_, m) in zip(w, pairs)) % K.n for i in range(count)]
    finally:
        K.close()


def test_widths_beyond_the_pair_forms_are_refused(engine, knobs):
    from test_gpu_key_widths import Key
    K = Key(engine, 3212)
    L, R = K.L, K.R
    try:
        x = R.up([3, 5, 7], 2 * K.nw)
        out = ctypes.c_void_p()
        arr = (ctypes.c_void_p * 2)(x.value, x.value)
        assert L.pgpu_batch_ct_weighted_sum(K.pk._h, arr, 2, None, 0, ctypes.byref(out)) == UNSUPPORTED and not out.value
        assert b"pair" in L.pgpu_last_error()
        for bits in (3212, 4096):
            assert L.pgpu_ct_weighted_sum_plan(bits, 3, 2, None, 0, None, None, None, None, None) == UNSUPPORTED
    finally:
        K.close()


def test_launches_carry_the_wsum_kind(engine, knobs):
    """kind 10, form PGPU_FORM_SEQ; one launch for one slice, one more for the fold of several, as the plan query says"""
    c = Case(engine, 2048)
    rng = random.Random(12)
    L, R = c.L, c.R
    try:
        count, K = 9, 8
        hs = [c.encrypt([rng.randrange(c.n) for _ in range(count)], rng) for _ in range(K)]    # pair rows: no conversion launch
        xs = [R.down(h) for h in hs]
        w = [rng.getrandbits(16) | 1 for _ in range(K)]
        wa = R.i2l(w, 1)
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_set_timing(1) == 0
        try:
            for slices, launches in ((1, 1), (2, 2), (8, 2), (None, 2)):
                knobs(slices)
                sl = ctypes.c_int()
                assert L.pgpu_ct_weighted_sum_plan(2048, count, K, wa.ctypes.data_as(ctypes.c_void_p), 1, None, None,
                                                   ctypes.byref(sl), None, None) == 0
                assert (1 if sl.value == 1 else 2) == launches, slices
                assert L.pgpu_synchronize() == 0
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                   # drop what earlier calls left
                y = wsum(L, R, c.pk._h, hs, w)
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)               # (before the download, which may launch a conversion)
                assert n == launches, (slices, n)
                assert all(kinds[i] == KIND_WSUM and forms[i] == FORM_SEQ and ms[i] > 0 for i in range(n))
                assert R.down(y) == expect(xs, w, c.nsq)
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_refusals_are_host_side_and_launch_nothing(engine, knobs):
    """every refusal of the call but three: stale handles (a pool torn down and set up again) and pools of more than one
    GPU cannot be provoked inside one session on one GPU, and a schedule of 2^31 steps needs a weight of 256 MiB; they are
    NOT covered here (the last one is, on the host, by tests/cpp/wsum_policy_tests.cpp)"""
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(11)
    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    try:
        xp = c.encrypt([1, 2, 3, 4, 5, 6], rng)                                  # pair rows: no conversion launch on the way in
        xq = c.encrypt([6, 5, 4, 3, 2, 1], rng)
        short = c.encrypt([1, 2, 3, 4, 5], rng)
        narrow = R.up([3, 5, 7, 9, 11, 13], c.nw)
        c1 = Case(engine, 1024)
        x1 = c1.encrypt([1, 2, 3, 4, 5, 6], rng)
        p3, q3, hs3 = key_case(3072, True)
        pk3 = engine.PublicKey(p3 * q3, 3072, hs=hs3)
        xw = R.up([rng.randrange(1, c.nsq) for _ in range(6)], 2 * c.nw)
        p4, q4, _ = key_case(4096, False)
        pk4 = engine.PublicKey(p4 * q4, 4096)
        x4 = R.up([3, 5, 7, 9, 11, 13], 128)
        out = ctypes.c_void_p()
        wa = R.i2l([3, 5], 1)
        wp = wa.ctypes.data_as(ctypes.c_void_p)

        def call(key, hs, n_terms, weights, w_words, null_out=False):
            arr = (ctypes.c_void_p * max(1, len(hs)))(*[h.value if h is not None else None for h in hs]) if hs is not None else None
            return L.pgpu_batch_ct_weighted_sum(key, arr, n_terms, weights, w_words, None if null_out else ctypes.byref(out))
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                       # drop what earlier calls left
            k = c.pk._h
            invalid = [
                (None, [xp, xq], 2, wp, 1), (k, None, 2, wp, 1), (k, [xp, None], 2, wp, 1),       # null handles
                (k, [xp, xq], 0, wp, 1), (k, [xp, xq], 65536, wp, 1),                             # n_terms == 0, above the cap
                (k, [xp, short], 2, wp, 1), (k, [short, xp], 2, None, 0),                         # counts that differ
                (k, [xp, narrow], 2, wp, 1),                                                      # ciphertext width mismatch
                (k, [xp, x1], 2, wp, 1), (pk3._h, [xw, xw], 2, wp, 1),                            # a batch of another key
                (k, [xp, xq], 2, wp, 0), (k, [xp, xq], 2, wp, -1),                                # w_words < 1 with weights
            ]
            for args in invalid:
                assert call(*args) == INVALID, args[2:]
                assert not out.value
            assert call(k, [xp, xq], 2, wp, 1, null_out=True) == INVALID
            assert call(k, [xp, short], 2, wp, 1) == INVALID and b"Size mismatch" in L.pgpu_last_error()
            assert call(k, [xp, narrow], 2, wp, 1) == INVALID and b"width" in L.pgpu_last_error()
            # the masked table-gather policy: refused, and the text says why
            assert L.pgpu_set_table_gather_policy(1) == 0
            try:
                assert call(k, [xp, xq], 2, wp, 1) == UNSUPPORTED
                err = L.pgpu_last_error()
                assert b"masked" in err and b"plaintext weights" in err and not out.value
            finally:
                L.pgpu_set_table_gather_policy(0)
            # a key class without pair rows
            assert call(pk4._h, [x4, x4], 2, wp, 1) == UNSUPPORTED and b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0           # nothing was launched
        finally:
            L.pgpu_set_timing(0)
            c1.R.close()
        assert R.down(wsum(L, R, c.pk._h, [xp, xq], [3, 5])) == expect([R.down(xp), R.down(xq)], [3, 5], c.nsq)
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
x = R.up([3, 5, 7], 64)
arr = (ctypes.c_void_p * 2)(x.value, x.value)
out = ctypes.c_void_p()
rc = R.L.pgpu_batch_ct_weighted_sum(pk._h, arr, 2, None, 0, ctypes.byref(out))
print("rc", rc, R.L.pgpu_last_error().decode())
R.close()
sys.exit(0 if rc == -3 and not out.value else 1)
"""


@pytest.mark.parametrize("switch", ["PGPU_PAIR_ROWS", "PGPU_HENSEL"])
def test_refused_without_pair_rows(engine, switch):
    """PGPU_PAIR_ROWS=0 / PGPU_HENSEL=0 leave resident ciphertexts without a pair form: PGPU_ERR_UNSUPPORTED (own process:
    the switches are read once; the process is what the test is about)"""
    env = dict(os.environ, **{switch: "0"})
    r = subprocess.run([sys.executable, "-c", _NO_PAIR_ROWS, ROOT], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


def test_two_lanes_at_once(engine, knobs):
    """two threads on different batch lanes, each with its own inputs; one run.  An operand of the other thread's lane is
    ordered in by events: the result sits on the lane of xs[0]"""
    c = Case(engine, 2048)
    L = c.L
    results, errors = {}, []
    shared_vals = [random.Random(7).randrange(1, c.nsq) for _ in range(40)]
    shared = c.R.up(shared_vals, 2 * c.nw)                                       # lane 0, read by both threads

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            rng = random.Random(600 + lane)
            count, K = 40, 5
            xs = [[rng.randrange(1, c.nsq) for _ in range(count)] for _ in range(K)]
            hs = [R.up(x, 2 * c.nw) for x in xs]
            assert L.pgpu_batch_lane(hs[0]) == lane
            for it in range(2):
                w = [rng.getrandbits(24) for _ in range(K + 1)]
                y = wsum(L, R, c.pk._h, hs + [shared], w)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = (R.down(y), xs + [shared_vals], w)
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
        assert len(results) == 4
        for got, xs, w in results.values():
            assert got == expect(xs, w, c.nsq)
        assert c.R.down(shared) == shared_vals
    finally:
        c.R.close()


def test_python_weighted_sum(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(5)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    ms = [[rng.randrange(1 << 40) for _ in range(10)] for _ in range(4)]
    cts = [pk.encrypt(m, [rng.getrandbits(1024) for _ in m]) for m in ms]
    w = [rng.getrandbits(20), 0, 1, n - 3]
    assert sk.decrypt(pk.weighted_sum(cts, w)) == [sum(a * m[i] for a, m in zip(w, ms)) % n for i in range(10)]
    assert sk.decrypt(pk.weighted_sum(cts)) == [sum(m[i] for m in ms) % n for i in range(10)]
    for bad in (([], None), (cts, w[:-1]), (cts, [-1] + w[1:]), (cts[:2] + [cts[2][:-1]], None)):
        with pytest.raises(RuntimeError):
            pk.weighted_sum(*bad)
