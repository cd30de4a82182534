"""The bucket-method encrypted matvec on resident ciphertexts (pgpu_batch_ct_matvec_bucket; csrc/hensel_bucket.hpp) on the GPU:
    out[i] = prod_j x[j]^(w[i][j] mod 2^e_bits) mod n^2
held bit-identical to Python's pow for the 1024-, 2048- and 3072-bit key classes: a shape whose level-1 chains fill more
than one wavefront, forced windows and blocks (every path of the two reduction levels: level 1 alone, level 2 alone, both),
the same paths with more than 8192 chains under a 2048-bit key (the (4,18) form of the reductions beside the (8,9) one that
small launches take), the edge weights of tests/test_bucket_model.py, a full-width signed weight through CRT decrypt, the agreement with
pgpu_batch_ct_matvec, both input forms, chaining, two lanes at once, the refusals, the timing record and the Python
layer.  Everything is exact: there are no tolerances.  In the reference such a map is composed from
CipherText::operator* (ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72) term by term."""
import ctypes
import json
import os
import random
import subprocess
import sys
import threading

import pytest

from test_gpu_pair_rows import Res, key_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KIND_BUCKET, FORM_SEQ = 12, 2         # PGPU_KERNEL_BUCKET, PGPU_FORM_SEQ (include/pgpu.h)
INVALID, UNSUPPORTED = -1, -3
BITS = [1024, 2048, 3072]


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


def bucket(L, R, key, x, weights, rows, e_bits, words=None):
    """one pgpu_batch_ct_matvec_bucket call; weights: rows * cols ints, row-major (bits above the words are cut off here)"""
    ww = words or (e_bits + 63) // 64
    wa = R.i2l([v & ((1 << (64 * ww)) - 1) for v in weights], ww)
    y = R.op(L.pgpu_batch_ct_matvec_bucket, key, x, wa.ctypes.data_as(ctypes.c_void_p), ww, rows, e_bits)
    wa[:] = 0xFFFFFFFFFFFFFFFF                                     # the weights are consumed before the call returns
    return y


def expect(x, weights, rows, e_bits, nsq):
    cols, mask = len(x), (1 << e_bits) - 1
    out = []
    for i in range(rows):
        acc = 1
        for j in range(cols):
            a = weights[i * cols + j] & mask
            if a:
                acc = acc * pow(x[j], a, nsq) % nsq
        out.append(acc)
    return out


def plan(L, bits, rows, cols, e_bits):
    c, b = ctypes.c_int(), ctypes.c_int()
    by, pr, de = ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    assert L.pgpu_ct_matvec_bucket_plan(bits, rows, cols, e_bits, ctypes.byref(c), ctypes.byref(b), ctypes.byref(by),
                                        ctypes.byref(pr), ctypes.byref(de)) == 0
    return c.value, b.value, by.value, pr.value, de.value


def edge_weights(e_bits, c, rng, count):
    """as tests/test_bucket_model.py: 0, 2^e_bits - 1, 1, 2^(c t) at the window boundaries, bits above e_bits, random"""
    ws = [0, (1 << e_bits) - 1, 1]
    ws += [1 << (c * t) for t in range((e_bits + c - 1) // c)]
    ws += [(1 << (e_bits + 3)) | (1 << e_bits) | rng.getrandbits(e_bits)]
    while len(ws) < count:
        ws.append(rng.getrandbits(e_bits))
    return ws


# ---- the reductions in the key's own (4,18) form: more than 8192 chains under a 2048-bit-class key ----
WIDE_MAX_CHAINS = 8192                # policy::segsum_wide_pays(8, chains): ceil(chains / 8) <= kSimds = 1024 wavefronts
BASE_COLS = 8
# (c, b, e_bits, rows), and which form level 1 / level 2 must run in ("base": (4,18), "wide": (8,9), None: no such launch)
BASE_SHAPES = {
    1: ((2, 4, 61, 265), ("base", None)),     # level 1 alone: 8215 chains of length 4, nb = 1; W = 31, top window one bit
    2: ((2, 1, 61, 265), (None, "base")),     # level 2 alone: 8215 chains of length 4, n_sqr = n_mul = 0
    3: ((4, 4, 59, 547), ("base", "base")),   # 32820 and 8205 chains of length 4; W = 15, top window 3 bits, n_sqr 2, n_mul 4
    4: ((8, 4, 49, 19), ("base", "wide")),    # 133 x 64 = 8512 chains of length 4, then 133 of length 64: one call, two forms
}


def reduce_chains(rows, e_bits, c, b):
    """(W, [level 1, level 2]) with a level as (chains, length) or None, as pgpu_batch_ct_matvec_bucket launches them"""
    W, nb = (e_bits + c - 1) // c, (1 << c) // b
    return W, [(rows * W * nb, b) if b > 1 else None, (rows * W, nb) if nb > 1 else None]


def wide_pays(L, bits, chains):
    """the policy's own word on a launch of this many chains (pack_wide_pays is segsum_wide_pays while PGPU_PACK_WIDE is unset)"""
    lanes, limbs = ctypes.c_int(), ctypes.c_int()
    assert L.pgpu_ct_pack_plan(bits, chains, 3, 11, ctypes.byref(lanes), ctypes.byref(limbs), None) == 0
    assert (lanes.value, limbs.value) in ((4, 18), (8, 9))
    return lanes.value == 8


def cyclic_weights(rows, cols, e_bits, c, rng):
    """many output rows for the price of eight references: seven non-zero weight rows that hold every edge weight of
    edge_weights() and random ones, and the all-zero row.  The rows of the call cycle through five of the eight -- five is
    coprime to the 16 chains of a wavefront, so that every position in a wavefront meets every one of them --; row 0, the
    middle row and the last row each have a weight row that no other row has.  Returns (table, pick): the distinct weight
    rows and the number of the one that row i uses"""
    ws = edge_weights(e_bits, c, rng, 7 * cols)
    assert len(ws) == 7 * cols, "every edge weight must find a place"
    t = [ws[k * cols:(k + 1) * cols] for k in range(7)]
    table = [t[0], [0] * cols, t[1], t[2], t[3], t[4], t[5], t[6]]
    pick = [i % 5 for i in range(rows)]
    pick[0], pick[rows // 2], pick[rows - 1] = 5, 6, 7
    return table, pick


def base_form_shape(L, R, key, bits, nsq, x, xv, shape, rng):
    """one of BASE_SHAPES on the resident x (its values xv), with PGPU_BUCKET_WINDOW / _BLOCK forced to the shape's (c, b)
    by the caller: the plan is the shape's, every reduction level is on its side of the threshold -- by the count and by
    the policy's own answer --, the call's rows equal pow().  Returns (y, table, pick)"""
    (c, b, e_bits, rows), sides = BASE_SHAPES[shape]
    cols = len(xv)
    pc, pb, nbytes = plan(L, bits, rows, cols, e_bits)[:3]
    assert (pc, pb) == (c, b)
    W, levels = reduce_chains(rows, e_bits, pc, pb)
    assert nbytes == rows * W * (1 << c) * 576 <= 80 << 20
    for lv, side in zip(levels, sides):
        assert (lv is None) == (side is None), (shape, lv, side)
        if lv:
            chains, length = lv
            print("shape", shape, "chains", chains, "of length", length, side)
            assert (chains <= WIDE_MAX_CHAINS) == (side == "wide") == wide_pays(L, bits, chains), (shape, chains)
            assert length >= 4                                                   # the main loop iterates
            if shape != 4:
                assert chains % 16                                               # the last wavefront has idle groups
    assert levels[1] is None or levels[1][0] % 8                                 # ... also in the wide form
    table, pick = cyclic_weights(rows, cols, e_bits, c, rng)
    assert len({tuple(r) for r in table}) == 8 and all(pick.count(k) == 1 for k in (5, 6, 7)) and table[1] == [0] * cols
    w = [v for i in range(rows) for v in table[pick[i]]]
    y = bucket(L, R, key, x, w, rows, e_bits, words=(e_bits + 3) // 64 + 1)      # (room for the bits above e_bits)
    assert L.pgpu_batch_count(y) == rows and L.pgpu_batch_row_limbs(y) == 144
    want = [expect(xv, r, 1, e_bits, nsq)[0] for r in table]                     # once per distinct weight row
    assert want[1] == 1 and len(set(want)) == 8
    got = R.down(y)
    bad = [i for i in range(rows) if got[i] != want[pick[i]]]
    assert not bad, (shape, len(bad), bad[:20])
    return y, table, pick


@pytest.fixture
def knobs(monkeypatch):
    names = ("PGPU_BUCKET_WINDOW", "PGPU_BUCKET_BLOCK", "PGPU_SEGSUM_CHUNK")
    monkeypatch.delenv("PGPU_PACK_WIDE", raising=False)           # (wide_pays asks the pack plan for the policy's threshold)
    for name in names:
        monkeypatch.delenv(name, raising=False)

    def force(window=None, block=None, chunk=None):
        for name, v in zip(names, (window, block, chunk)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


@pytest.mark.parametrize("bits", BITS)
def test_chain_count_shape_and_default_plans(engine, knobs, bits):
    """3 x 67 at 13 bits with c = 4 forced: W = 4, b = 4, 48 level-1 chains -- more than one wavefront at (4,18) and
    (8,14), a partly filled last one at (2,19) --, empty and multi-entry buckets; then 1 x 1 and 2 x 300 as the plan
    has them"""
    c = Case(engine, bits)
    rng = random.Random(bits)
    L, R = c.L, c.R
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(300)], rng)           # resident DJN encrypt: pair rows
        xv = R.down(x)
        x67 = c.encrypt([rng.randrange(c.n) for _ in range(67)], rng)
        x67v = R.down(x67)
        knobs(4)
        assert plan(L, bits, 3, 67, 13)[:2] == (4, 4)
        w = [rng.getrandbits(13) for _ in range(3 * 67)]
        y = bucket(L, R, c.pk._h, x67, w, 3, 13)
        assert L.pgpu_batch_count(y) == 3 and L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(x67) > 0
        assert L.pgpu_batch_lane(y) == L.pgpu_batch_lane(x67)
        assert R.down(y) == expect(x67v, w, 3, 13, c.nsq)
        knobs()
        x1 = c.encrypt([rng.randrange(c.n)], rng)
        for wv in (0, 1, 0xDEADBEEF):
            assert R.down(bucket(L, R, c.pk._h, x1, [wv], 1, 32)) == expect(R.down(x1), [wv], 1, 32, c.nsq)
        w = [rng.getrandbits(32) for _ in range(2 * 300)]
        assert R.down(bucket(L, R, c.pk._h, x, w, 2, 32)) == expect(xv, w, 2, 32, c.nsq)
        assert R.down(x) == xv and R.down(x67) == x67v                          # the inputs are unchanged
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_forced_plans(engine, knobs, bits):
    """c in {1, 2, 3, 5, 8} x b in {1, 2, default, 2^c} on 2 x 40 at e_bits in {1, 13, 32, 65}: level 2 alone (b = 1),
    level 1 alone (b = 2^c), both; W = 1 and a narrower top window"""
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    L, R = c.L, c.R
    try:
        x = R.up([rng.randrange(1, c.nsq) for _ in range(40)], 2 * c.nw)
        xv = R.down(x)
        for e_bits in (1, 13, 32, 65):
            w = [rng.getrandbits(e_bits) for _ in range(80)]
            want = expect(xv, w, 2, e_bits, c.nsq)                              # once, shared by every plan
            for cw in (1, 2, 3, 5, 8):
                for b in sorted({1, 2, 1 << ((cw + 1) // 2), 1 << cw}):
                    knobs(cw, b)
                    assert plan(L, bits, 2, 40, e_bits)[:2] == (cw, b)
                    assert R.down(bucket(L, R, c.pk._h, x, w, 2, e_bits)) == want, (e_bits, cw, b)
    finally:
        R.close()


@pytest.mark.parametrize("shape", sorted(BASE_SHAPES))
def test_reductions_in_the_base_form(engine, knobs, shape):
    """bucket_reduce_kernel has four instantiations (k_hensel.hip parts 63-66), and a 2048-bit-class key runs the reductions
    of small calls in the wide one:
      <2,19>  part 63  every test of this module at 1024 bits (the class has no wide form)
      <8,14>  part 65  every test of this module at 3072 bits (likewise)
      <8,9>   part 66  every test of this module at 2048 bits but this one -- none of their launches has more than 8192
                       chains --, and level 2 of shape 4 here
      <4,18>  part 64  this test (shapes 1-4 of BASE_SHAPES), test_launches_of_one_call_in_two_forms, and
                       test_gpu_key_widths.py::test_bucket_reductions_in_both_forms at the first and the last width of the class
    Each shape derives its chain counts from the plan's (c, b) and asserts on which side of the threshold every level
    falls (base_form_shape); the counts leave idle groups in the last wavefront, except level 1 of shape 4 (8512 = 532 x 16).
    The accumulation levels of these shapes run in (4,18) as well, the Horner launch over the rows in (8,9).  x is
    uploaded words with the ends of the value range in the first four columns; shape 1 runs a second time on pair rows
    from a resident DJN encrypt and goes through CRT decrypt"""
    c = Case(engine, 2048)
    rng = random.Random(6400 + shape)
    L, R = c.L, c.R
    (cw, b, e_bits, _), _ = BASE_SHAPES[shape]
    try:
        knobs(cw, b)
        xv = [1, c.nsq - 1, c.n + 1, c.nsq - c.n + 1] + [rng.randrange(1, c.nsq) for _ in range(BASE_COLS - 4)]
        x = R.up(xv, 2 * c.nw)
        base_form_shape(L, R, c.pk._h, 2048, c.nsq, x, xv, shape, rng)
        assert R.down(x) == xv                                                   # the input is unchanged
        if shape == 1:
            m = [rng.randrange(c.n) for _ in range(BASE_COLS)]
            xp = c.encrypt(m, rng)
            assert L.pgpu_batch_row_limbs(xp) == 144
            y, table, pick = base_form_shape(L, R, c.pk._h, 2048, c.nsq, xp, R.down(xp), shape, rng)
            mask = (1 << e_bits) - 1
            plain = [sum((w & mask) * v for w, v in zip(r, m)) % c.n for r in table]
            assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, y)) == [plain[k] for k in pick]
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_edge_weights(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    L, R = c.L, c.R
    try:
        for cw, e_bits in ((4, 13), (3, 32), (8, 65), (None, 64)):
            knobs(cw)
            ws = edge_weights(e_bits, cw or plan(L, bits, 2, 1, e_bits)[0], rng, 0)
            cols = len(ws)
            x = c.encrypt([rng.randrange(c.n) for _ in range(cols)], rng)
            w = ws + [0] * cols                                                  # row 1: all zero -> the ciphertext 1
            got = R.down(bucket(L, R, c.pk._h, x, w, 2, e_bits, words=(e_bits + 3) // 64 + 1))   # (room for the bits above e_bits)
            assert got == expect(R.down(x), w, 2, e_bits, c.nsq), (cw, e_bits)
            assert got[1] == 1
    finally:
        R.close()


def test_signed_round_trip(engine, knobs):
    """the full-width weight n - 1 (that is -1 mod n) on 3 columns: decrypt gives -sum(m) mod n"""
    c = Case(engine, 2048)
    rng = random.Random(5)
    L, R = c.L, c.R
    try:
        m = [rng.randrange(c.n) for _ in range(3)]
        x = c.encrypt(m, rng)
        w = [c.n - 1] * 3
        y = bucket(L, R, c.pk._h, x, w, 1, c.n.bit_length())
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, y)) == [-sum(m) % c.n]
        assert R.down(y) == expect(R.down(x), w, 1, c.n.bit_length(), c.nsq)
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_against_matvec_input_forms_and_chaining(engine, knobs, bits):
    """the same resident x through pgpu_batch_ct_matvec: equal downloads; x as pair rows and as uploaded words; the
    result feeds CT + CT and CRT decrypt"""
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    try:
        rows, cols, e_bits = 3, 50, 32
        m = [rng.randrange(c.n) for _ in range(cols)]
        xp = c.encrypt(m, rng)                                                   # pair rows
        xv = R.down(xp)
        xw = R.up(xv, 2 * c.nw)                                                  # the same ciphertexts as uploaded words
        w = [rng.getrandbits(e_bits) for _ in range(rows * cols)]
        wb = R.up(w, 1)
        ref = R.down(R.op(L.pgpu_batch_ct_matvec, c.pk._h, xp, wb, rows, e_bits))
        yp = bucket(L, R, c.pk._h, xp, w, rows, e_bits)
        yw = bucket(L, R, c.pk._h, xw, w, rows, e_bits)
        assert R.down(yp) == ref == R.down(yw)
        assert L.pgpu_batch_row_limbs(yw) == L.pgpu_batch_row_limbs(yp) > 0
        assert R.down(xw) == xv
        plain = [sum(w[i * cols + j] * m[j] for j in range(cols)) % c.n for i in range(rows)]
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, yp)) == plain
        s = R.op(L.pgpu_batch_ct_add, c.pk._h, yp, yw)
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, s)) == [2 * v % c.n for v in plain]
    finally:
        R.close()


def test_two_lanes_at_once(engine, knobs):
    c = Case(engine, 2048)
    L = c.L
    results, errors = {}, []

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            rng = random.Random(700 + lane)
            cols, rows = 90, 2
            xv = [rng.randrange(1, c.nsq) for _ in range(cols)]
            x = R.up(xv, 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for it in range(2):
                w = [rng.getrandbits(24) for _ in range(rows * cols)]
                y = bucket(L, R, c.pk._h, x, w, rows, 24)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = (R.down(y), xv, w, rows)
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
        for got, xv, w, rows in results.values():
            assert got == expect(xv, w, rows, 24, c.nsq)
    finally:
        c.R.close()


def test_refusals_are_host_side_and_launch_nothing(engine, knobs):
    """every refusal of the call but two, each by its message: stale handles (a pool torn down and set up again) and pools
    of more than one GPU cannot be provoked inside one session on one GPU; they are NOT covered here.  The batches of
    another key have this key's width (a second 2048-bit modulus, tests/golden/aggregate_refusals.json), once in pair rows
    and once in Montgomery form, so that they pass the width check and reach agg_admit"""
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(11)
    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    try:
        xs = [rng.randrange(1, c.nsq) for _ in range(6)]
        xp = c.encrypt([1, 2, 3, 4, 5, 6], rng)                                  # pair rows: no conversion launch on the way in
        narrow = R.up([3, 5, 7, 9, 11, 13], c.nw)
        wide = R.up(xs, 2 * c.nw + 1)
        other = engine.PublicKey(int(json.load(open(os.path.join(ROOT, "tests", "golden", "aggregate_refusals.json")))["other_n"]["2048"], 16), 2048)
        pair_other = R.op(L.pgpu_batch_ct_add, other._h, R.up(xs, 2 * c.nw), R.up(xs, 2 * c.nw))
        L.pgpu_debug_set_hensel(0)
        try:
            mont_other = R.op(L.pgpu_batch_ct_add, other._h, R.up(xs, 2 * c.nw), R.up(xs, 2 * c.nw))
        finally:
            L.pgpu_debug_set_hensel(1)
        assert L.pgpu_batch_row_limbs(pair_other) > 0 and L.pgpu_batch_is_montgomery(mont_other) == 1
        assert L.pgpu_batch_words(pair_other) == L.pgpu_batch_words(mont_other) == 2 * c.nw
        p4, q4, _ = key_case(4096, False)
        pk4 = engine.PublicKey(p4 * q4, 4096)
        x4 = R.up([3, 5, 7, 9, 11, 13], 128)
        big = R.up([3] * 4096, 2 * c.nw)                                         # (uploaded words; converted only after admission)
        out = ctypes.c_void_p()
        wa = R.i2l([3, 5, 7, 9, 11, 13], 1)
        wp = wa.ctypes.data_as(ctypes.c_void_p)
        wbig = R.i2l([1] * (8192 * 6), 1)
        wbp = wbig.ctypes.data_as(ctypes.c_void_p)

        def call(key, x, w, w_words, rows, e_bits, null_out=False):
            return L.pgpu_batch_ct_matvec_bucket(key, x, w, w_words, rows, e_bits, None if null_out else ctypes.byref(out))
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                       # drop what the set-up left
            k = c.pk._h
            invalid = [
                ((None, xp, wp, 1, 1, 32), b"null"), ((k, None, wp, 1, 1, 32), b"null"), ((k, xp, None, 1, 1, 32), b"null"),
                ((k, xp, wp, 1, 0, 32), b"rows must be positive"),
                ((k, xp, wp, 0, 1, 32), b"w_words must be positive"), ((k, xp, wp, -1, 1, 32), b"w_words must be positive"),
                ((k, xp, wp, 1, 1, 0), b"e_bits outside"), ((k, xp, wp, 1, 1, 65), b"e_bits outside"), ((k, xp, wp, 1, 1, -3), b"e_bits outside"),
                ((k, narrow, wp, 1, 1, 32), b"ciphertext width mismatch"), ((k, wide, wp, 1, 1, 32), b"ciphertext width mismatch"),
                ((k, pair_other, wp, 1, 1, 32), b"different key"), ((k, mont_other, wp, 1, 1, 32), b"different key")]
            for args, text in invalid:
                assert call(*args) == INVALID, args[3:]
                assert text in L.pgpu_last_error() and not out.value, (args[3:], L.pgpu_last_error())
            assert call(k, xp, wp, 1, 1, 32, null_out=True) == INVALID and b"null" in L.pgpu_last_error()
            knobs(10)
            # rows * W * cols at 2^31: 2^19 rows of one window over 4096 columns (the weights are not read before the refusal)
            assert call(k, big, wbp, 1, 1 << 19, 1) == INVALID and b"2^31" in L.pgpu_last_error() and not out.value
            # rows * W * 2^c at 2^31: 2^21 rows x 1 window x 2^10 buckets over 6 columns
            assert call(k, xp, wbp, 1, 1 << 21, 1) == INVALID and b"2^31" in L.pgpu_last_error() and not out.value
            # a forced window is not held against the plan's cap, but the bucket block is bounded before anything is allocated:
            # 8192 rows x 1 window x 2^10 buckets of 576 bytes are 4.5 GiB
            assert call(k, xp, wbp, 1, 8192, 1) == INVALID and b"exceeds 4 GiB" in L.pgpu_last_error() and not out.value
            knobs()
            # the masked table-gather policy: refused, and the text says why
            assert L.pgpu_set_table_gather_policy(1) == 0
            try:
                assert call(k, xp, wp, 1, 1, 32) == UNSUPPORTED
                err = L.pgpu_last_error()
                assert b"bucket matvec" in err and b"masked" in err and b"digits of the plaintext weights" in err and not out.value
            finally:
                L.pgpu_set_table_gather_policy(0)
            # a key class without pair rows
            assert call(pk4._h, x4, wp, 1, 1, 32) == UNSUPPORTED and b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0           # nothing was launched
        finally:
            L.pgpu_set_timing(0)
        w = [3, 5, 7, 9, 11, 13]
        assert R.down(bucket(L, R, c.pk._h, xp, w, 1, 32)) == expect(R.down(xp), w, 1, 32, c.nsq)
        # the plan query refuses what it cannot plan
        assert L.pgpu_ct_matvec_bucket_plan(2048, 0, 5, 32, None, None, None, None, None) == INVALID
        assert L.pgpu_ct_matvec_bucket_plan(2048, 1, 5, 0, None, None, None, None, None) == INVALID
        assert L.pgpu_ct_matvec_bucket_plan(4096, 1, 5, 32, None, None, None, None, None) == UNSUPPORTED
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
w = R.i2l([1, 2, 3], 1)
out = ctypes.c_void_p()
rc = R.L.pgpu_batch_ct_matvec_bucket(pk._h, x, w.ctypes.data_as(ctypes.c_void_p), 1, 1, 8, ctypes.byref(out))
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


def test_launches_carry_the_bucket_kind(engine, knobs):
    """kind 12, form PGPU_FORM_SEQ; accumulation levels + reduce launches + the Horner launch, for three forced plans:
    (c, b, segsum chunk) over 2 x 40 -- a bucket holds at most 40 columns, so chunk 64 gives one level and chunk 2 up to
    six (ceil(log2 of the fullest bucket)), counted here from the weights"""
    c = Case(engine, 2048)
    rng = random.Random(12)
    L, R = c.L, c.R
    try:
        rows, cols = 2, 40
        x = c.encrypt([rng.randrange(c.n) for _ in range(cols)], rng)           # pair rows: no conversion launch
        xv = R.down(x)
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_set_timing(1) == 0
        try:
            # (c, b, chunk, e_bits): both levels + Horner; level 1 alone, W == 1; level 2 alone + Horner, several accumulation levels
            for cw, b, chunk, e_bits in ((4, 4, 64, 13), (3, 8, 64, 3), (2, 1, 2, 13)):
                knobs(cw, b, chunk)
                w = [rng.getrandbits(e_bits) for _ in range(rows * cols)]
                W = (e_bits + cw - 1) // cw
                fullest = max(sum(1 for j in range(cols) if (w[i * cols + j] >> (cw * t)) & ((1 << cw) - 1) == d)
                              for i in range(rows) for t in range(W) for d in range(1, 1 << cw))
                levels = 1
                while fullest > chunk:
                    fullest = (fullest + chunk - 1) // chunk
                    levels += 1
                reduces = (1 if b > 1 else 0) + (1 if (1 << cw) // b > 1 else 0)
                launches = levels + reduces + (1 if W > 1 else 0)
                assert L.pgpu_synchronize() == 0
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                   # drop what earlier calls left
                y = bucket(L, R, c.pk._h, x, w, rows, e_bits)
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)               # (before the download, which may launch a conversion)
                assert n == launches, (cw, b, chunk, n, launches)
                assert all(kinds[i] == KIND_BUCKET and forms[i] == FORM_SEQ and ms[i] > 0 for i in range(n))
                assert R.down(y) == expect(xv, w, rows, e_bits, c.nsq)
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_launches_of_one_call_in_two_forms(engine, knobs):
    """shape 4 of BASE_SHAPES: level 1 in (4,18), level 2 in (8,9) within one call.  A bucket holds at most the 8 columns, so
    chunk 64 gives one accumulation level: 1 + 2 reduces + the Horner launch, every one -- the base-form one included --
    recorded once, with kind 12 and form PGPU_FORM_SEQ"""
    c = Case(engine, 2048)
    rng = random.Random(13)
    L, R = c.L, c.R
    (cw, b, e_bits, rows), sides = BASE_SHAPES[4]
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(BASE_COLS)], rng)       # pair rows: no conversion launch
        xv = R.down(x)
        knobs(cw, b, 64)
        W, levels = reduce_chains(rows, e_bits, *plan(L, 2048, rows, BASE_COLS, e_bits)[:2])
        assert W > 1 and sides == ("base", "wide")
        assert [wide_pays(L, 2048, lv[0]) for lv in levels] == [False, True]
        table, pick = cyclic_weights(rows, BASE_COLS, e_bits, cw, rng)
        w = [v for i in range(rows) for v in table[pick[i]]]
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_set_timing(1) == 0
        try:
            assert L.pgpu_synchronize() == 0
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                       # drop what the set-up left
            y = bucket(L, R, c.pk._h, x, w, rows, e_bits)
            assert L.pgpu_synchronize() == 0
            n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                   # (before the download, which may launch a conversion)
            assert n == 1 + 2 + 1, n
            assert all(kinds[i] == KIND_BUCKET and forms[i] == FORM_SEQ and ms[i] > 0 for i in range(n))
        finally:
            L.pgpu_set_timing(0)
        want = [expect(xv, r, 1, e_bits, c.nsq)[0] for r in table]
        assert R.down(y) == [want[k] for k in pick]
    finally:
        R.close()


def test_python_matvec_bucket(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(5)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    m = [rng.randrange(1 << 40) for _ in range(12)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    w = [[rng.getrandbits(20) for _ in m], [0] * len(m), [n - 1] + [1] * (len(m) - 1)]
    got = pk.matvec_bucket(ct, w)
    assert got == pk.matvec(ct, w)
    assert sk.decrypt(got) == [sum(a * b for a, b in zip(r, m)) % n for r in w]
    assert pk.matvec_bucket(ct, w[0]) == got[:1]                                 # one flat row: a dot product
    for bad in (([], w[0]), (ct, w[0][:-1]), (ct, [w[0], w[1][:-1]])):
        with pytest.raises(RuntimeError, match="Size mismatch"):
            pk.matvec_bucket(*bad)
    with pytest.raises(RuntimeError, match="negative weights have no encoding"):
        pk.matvec_bucket(ct, [-1] + w[0][1:])
