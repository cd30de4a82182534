"""The encrypted segmented sum on resident ciphertexts (pgpu_batch_ct_segment_sum; csrc/hensel_segsum.hpp) on the GPU:
    out[g * n_segments + s] = prod_{ j : ids[g * cols + j] == s } x[j] mod n^2
held bit-identical to Python integers for the 1024-, 2048- and 3072-bit key classes: every shape class (one element,
segments of one element, one long segment, several groups, skewed groupings with empty segments and left-out elements),
forced chunks that reach every level boundary, edge ciphertexts, inputs in every form a resident ciphertext batch can
have, the round trip through CRT decrypt, the 0/1 matrix-vector route, chaining, two lanes at once, the timing record and
the refusals.  In the reference this sum is composed from CipherText::operator+ (ipcl/ciphertext.cpp:35-72) after a
gather on the host."""
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
NONE = 0xFFFFFFFF
KIND_SEGSUM, FORM_SEQ = 6, 2         # PGPU_KERNEL_SEGSUM, PGPU_FORM_SEQ (include/pgpu.h)
SHAPES = [(1, 1, 1), (7, 3, 1), (33, 5, 2), (64, 64, 1), (65, 1, 1), (300, 9, 3)]      # (cols, n_segments, groups)


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

    def segsum(self, x, ids, groups, n_segments):
        a = np.array(ids, dtype=np.uint32)
        assert len(a) == groups * self.L.pgpu_batch_count(x)
        h = self.R.op(self.L.pgpu_batch_ct_segment_sum, self.pk._h, x, a.ctypes.data_as(ctypes.c_void_p), groups, n_segments)
        a[:] = 12345                                            # ids may be reused as soon as the call returns
        return h

    def expect(self, xs, ids, groups, n_segments):
        cols = len(xs)
        out = [1] * (groups * n_segments)
        for g in range(groups):
            for j in range(cols):
                s = ids[g * cols + j]
                if s != NONE:
                    out[g * n_segments + s] = out[g * n_segments + s] * xs[j] % self.nsq
        return out


@pytest.fixture
def knobs(monkeypatch):
    monkeypatch.delenv("PGPU_SEGSUM_CHUNK", raising=False)

    def force(c=None):
        if c is None:
            monkeypatch.delenv("PGPU_SEGSUM_CHUNK", raising=False)
        else:
            monkeypatch.setenv("PGPU_SEGSUM_CHUNK", str(c))
    return force


def make_ids(rng, cols, n_segments, groups):
    if (cols, n_segments) == (64, 64):
        return [j for j in range(cols)]                        # every segment has length 1
    if (cols, n_segments, groups) == (300, 9, 3):              # skewed: most of a group in one segment, segments 5 and 7 empty,
        pool = [0, 1, 2, 3, 4, 6, 8]                           # some elements left out
        return [NONE if rng.random() < 0.1 else (g if rng.random() < 0.8 else rng.choice(pool))
                for g in range(groups) for _ in range(cols)]
    return [rng.randrange(n_segments) for _ in range(groups * cols)]


@pytest.mark.parametrize("bits", BITS)
def test_segment_sum_is_exact_at_every_shape(engine, knobs, bits):
    """x from a resident DJN encrypt; the chunk the policy picks"""
    c = Case(engine, bits)
    rng = random.Random(bits)
    try:
        for cols, n_segments, groups in SHAPES:
            x = c.encrypt([rng.randrange(c.n) for _ in range(cols)], rng)
            xs = c.R.down(x)
            ids = make_ids(rng, cols, n_segments, groups)
            y = c.segsum(x, ids, groups, n_segments)
            assert c.L.pgpu_batch_count(y) == groups * n_segments
            assert c.L.pgpu_batch_row_limbs(y) == c.L.pgpu_batch_row_limbs(x) > 0 and c.L.pgpu_batch_lane(y) == c.L.pgpu_batch_lane(x)
            want = c.expect(xs, ids, groups, n_segments)
            assert c.R.down(y) == want, (cols, n_segments, groups)
            if (cols, n_segments, groups) == (300, 9, 3):
                assert want[5] == 1 and want[9 + 7] == 1           # the empty segments download as 1
            c.R.close()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_forced_chunks_reach_every_level(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    L = c.L
    try:
        cols = 70                                                  # (chunk 64: segments of 64 and 65 elements need 65 + 5 ...)
        xs = [rng.randrange(1, c.nsq) for _ in range(cols)]
        x = c.R.up(xs, 2 * c.nw)
        for chunk in (2, 3, 64):
            knobs(chunk)
            got_chunk, got_levels = ctypes.c_int(), ctypes.c_int()
            assert L.pgpu_ct_segment_sum_plan(bits, 37, 2, 37, ctypes.byref(got_chunk), ctypes.byref(got_levels)) == 0
            assert got_chunk.value == chunk
            if chunk == 2:
                assert got_levels.value >= 5                       # 37 -> 19 -> 10 -> 5 -> 3 -> 2 -> 1
            ids = [0] * 37 + [NONE] * (cols - 37)                  # (37, 2, 1): one segment of 37, one empty
            assert c.R.down(c.segsum(x, ids, 1, 2)) == c.expect(xs, ids, 1, 2), chunk
            # segments of exactly chunk, chunk + 1 and chunk^2 + 1 elements (the level boundaries), as three groups
            for m in (chunk, chunk + 1, chunk * chunk + 1):
                if m > cols:
                    continue
                ids = ([1] * m + [0] * (cols - m)) + ([NONE] * (cols - m) + [1] * m) + [j % 2 for j in range(cols)]
                assert c.R.down(c.segsum(x, ids, 3, 2)) == c.expect(xs, ids, 3, 2), (chunk, m)
            # a count of chunks that is no multiple of 64/G: 11 segments of 6 and 7 elements
            ids = [j % 11 for j in range(cols)]
            assert c.R.down(c.segsum(x, ids, 1, 11)) == c.expect(xs, ids, 1, 11), chunk
            c.R.close()
            x = c.R.up(xs, 2 * c.nw)
        if bits == 2048:                                           # chunk^2 + 1 for chunk 64, once
            knobs(64)
            big = [rng.randrange(1, c.nsq) for _ in range(64 * 64 + 1)]
            xb = c.R.up(big, 2 * c.nw)
            want = 1
            for v in big:
                want = want * v % c.nsq
            assert c.R.down(c.segsum(xb, [0] * len(big), 1, 1)) == [want]
    finally:
        c.R.close()


def test_plan_image_beyond_the_bounce_buffer(engine, knobs):
    """many groupings of few ciphertexts: the sorted list and the descriptors (over 256 KiB) reach the device through a
    worker lane's staging buffers instead of the calling thread's bounce buffer.  That choice is written once
    (csrc/capi_aggregate.inc: upload_plan_image) for the four calls that upload a plan image -- segment sum, spmv, weighted
    sum, segment scan -- so this case exercises the large path of all of them"""
    c = Case(engine, 1024)
    rng = random.Random(12)
    try:
        cols, n_segments, groups = 257, 3, 260
        xs = [rng.randrange(1, c.nsq) for _ in range(cols)]
        x = c.R.up(xs, 2 * c.nw)
        ids = [rng.randrange(n_segments) for _ in range(groups * cols)]
        assert c.R.down(c.segsum(x, ids, groups, n_segments)) == c.expect(xs, ids, groups, n_segments)
    finally:
        c.R.close()


def test_levels_on_both_sides_of_the_wide_form_threshold(engine, knobs):
    """2048-bit keys run a level of at most 8192 chains with 8 lanes per chain, a larger one with 4: many groupings of few
    ciphertexts put level 0 (and, with chunk 2, the first fold) above the threshold and the last folds below it"""
    c = Case(engine, 2048)
    rng = random.Random(13)
    try:
        cols, n_segments, groups = 192, 64, 130
        xs = [rng.randrange(1, c.nsq) for _ in range(cols)]
        x = c.R.up(xs, 2 * c.nw)
        ids = [j % n_segments for _ in range(groups) for j in range(cols)]          # 8320 segments of 3 elements
        want = c.expect(xs, ids, groups, n_segments)
        assert c.R.down(c.segsum(x, ids, groups, n_segments)) == want                # one level of 8320 chains
        knobs(2)
        assert c.R.down(c.segsum(x, ids, groups, n_segments)) == want                # 16640 chains, then 8320
        ids = [0] * cols + ids[cols:]                                                # ... and one long segment: 8 levels
        assert c.R.down(c.segsum(x, ids, groups, n_segments)) == c.expect(xs, ids, groups, n_segments)
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_edge_values(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    try:
        xs = [1, c.nsq - 1, 1, c.nsq - 1, c.nsq - 1] + [rng.randrange(1, c.nsq) for _ in range(6)]
        cols = len(xs)
        x = c.R.up(xs, 2 * c.nw)
        for ids, groups, n_segments in (([0, 0, 1, 1, 2] + [rng.randrange(3) for _ in range(6)], 1, 3),
                                        ([NONE] * (2 * cols), 2, 4),              # every output downloads as 1
                                        ([0] * cols, 1, 3)):                       # one group all in segment 0
            got = c.R.down(c.segsum(x, ids, groups, n_segments))
            assert got == c.expect(xs, ids, groups, n_segments)
        assert c.R.down(c.segsum(x, [NONE] * (2 * cols), 2, 4)) == [1] * 8
        assert c.R.down(c.segsum(x, [0] * cols, 1, 3))[1:] == [1, 1]
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_inputs_in_every_form_and_round_trip(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    try:
        cols, n_segments, groups = 45, 4, 2
        m = [rng.randrange(c.n) for _ in range(cols)]
        m2 = [rng.randrange(c.n) for _ in range(cols)]
        ids = [NONE if rng.random() < 0.1 else rng.randrange(n_segments) for _ in range(groups * cols)]
        x = c.encrypt(m, rng)                                   # resident DJN encrypt: pair rows
        xs = R.down(x)
        want = c.expect(xs, ids, groups, n_segments)
        assert R.down(c.segsum(x, ids, groups, n_segments)) == want
        assert R.down(c.segsum(R.up(xs, 2 * c.nw), ids, groups, n_segments)) == want     # uploaded plain ciphertext words
        x2 = c.encrypt(m2, rng)
        s = R.op(L.pgpu_batch_ct_add, c.pk._h, x, x2)           # a result of CT + CT
        y = c.segsum(s, ids, groups, n_segments)
        assert R.down(y) == c.expect(R.down(s), ids, groups, n_segments)
        # the round trip: decrypt(segment_sum(encrypt(m))) == the per-segment sums mod n
        d = R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, y))
        sums = [0] * (groups * n_segments)
        for g in range(groups):
            for j in range(cols):
                if ids[g * cols + j] != NONE:
                    sums[g * n_segments + ids[g * cols + j]] += m[j] + m2[j]
        assert d == [v % c.n for v in sums]
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_agrees_with_the_matvec_route(engine, knobs, bits):
    """what a caller can do today: pgpu_batch_ct_matvec with a 0/1 matrix and e_bits = 1"""
    c = Case(engine, bits)
    rng = random.Random(bits + 4)
    L, R = c.L, c.R
    try:
        cols, n_segments = 48, 6
        x = c.encrypt([rng.randrange(c.n) for _ in range(cols)], rng)
        ids = [rng.randrange(n_segments) for _ in range(cols)]
        w = R.up([1 if ids[j] == s else 0 for s in range(n_segments) for j in range(cols)], 1)
        mv = R.down(R.op(L.pgpu_batch_ct_matvec, c.pk._h, x, w, n_segments, 1))
        assert R.down(c.segsum(x, ids, 1, n_segments)) == mv
    finally:
        R.close()


def test_result_chains_into_every_operation(engine, knobs):
    c = Case(engine, 2048)
    rng = random.Random(78)
    L, R = c.L, c.R
    try:
        cols, n_segments = 40, 6
        m = [rng.randrange(c.n) for _ in range(cols)]
        x = c.encrypt(m, rng)
        ids = [rng.randrange(n_segments) for _ in range(cols)]
        y = c.segsum(x, ids, 1, n_segments)
        ys = R.down(y)
        assert ys == c.expect(R.down(x), ids, 1, n_segments)
        assert R.down(R.op(L.pgpu_batch_ct_add, c.pk._h, y, y)) == [v * v % c.nsq for v in ys]
        e = [rng.getrandbits(16) for _ in range(n_segments)]
        assert R.down(R.op(L.pgpu_batch_ct_mul, c.pk._h, y, R.up(e, 1), 16)) == [pow(v, k, c.nsq) for v, k in zip(ys, e)]
        pm = [rng.randrange(c.n) for _ in range(n_segments)]
        assert R.down(R.op(L.pgpu_batch_ct_add_plain, c.pk._h, y, R.up(pm, c.nw))) == \
            [v * (1 + c.n * k) % c.nsq for v, k in zip(ys, pm)]
        wm = [[rng.getrandbits(12) for _ in range(n_segments)] for _ in range(3)]
        z = R.op(L.pgpu_batch_ct_matvec, c.pk._h, y, R.up([v for row in wm for v in row], 1), 3, 12)
        want = []
        for row in wm:
            acc = 1
            for v, k in zip(ys, row):
                acc = acc * pow(v, k, c.nsq) % c.nsq
            want.append(acc)
        assert R.down(z) == want
        ids2 = [0, 1, 0, NONE, 1, 0]                            # a second segment sum (pooling) on the first one's result
        z2 = c.segsum(y, ids2, 1, 2)
        assert R.down(z2) == c.expect(ys, ids2, 1, 2)
        h = [sum(m[j] for j in range(cols) if ids[j] == s) for s in range(n_segments)]
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, z2)) == [(h[0] + h[2] + h[5]) % c.n, (h[1] + h[4]) % c.n]
    finally:
        R.close()


def test_two_lanes_at_once(engine, knobs):
    """two threads on different batch lanes, each with its own inputs; one run"""
    c = Case(engine, 2048)
    L = c.L
    results, errors = {}, []

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            rng = random.Random(600 + lane)
            cols, n_segments, groups = 90 + lane, 5, 2
            xs = [rng.randrange(1, c.nsq) for _ in range(cols)]
            x = R.up(xs, 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for it in range(2):
                ids = [rng.randrange(n_segments) for _ in range(groups * cols)]
                a = np.array(ids, dtype=np.uint32)
                y = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, x, a.ctypes.data_as(ctypes.c_void_p), groups, n_segments)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = (R.down(y), xs, ids, groups, n_segments)
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    ts = [threading.Thread(target=worker, args=(lane,)) for lane in (1, 2)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errors, errors
    assert len(results) == 4
    for got, xs, ids, groups, n_segments in results.values():
        assert got == c.expect(xs, ids, groups, n_segments)


def test_launches_carry_the_segsum_kind(engine, knobs):
    c = Case(engine, 2048)
    rng = random.Random(11)
    L, R = c.L, c.R
    try:
        knobs(4)
        x = c.encrypt([rng.randrange(c.n) for _ in range(50)], rng)       # pair rows already: no conversion launch
        xs = R.down(x)
        ids = [0] * 40 + [1] * 10                                          # chunk 4: 40 -> 10 -> 3 rows -> 1: three levels
        levels = ctypes.c_int()
        assert L.pgpu_ct_segment_sum_plan(2048, 50, 2, 40, None, ctypes.byref(levels)) == 0 and levels.value == 3
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                 # drop what earlier calls left
            y = c.segsum(x, ids, 1, 2)
            got = R.down(y)
            n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
        finally:
            L.pgpu_set_timing(0)
        assert got == c.expect(xs, ids, 1, 2)
        seg = [(kinds[i], forms[i]) for i in range(n) if kinds[i] == KIND_SEGSUM]
        assert len(seg) == levels.value                                    # one launch per level
        assert all(f == FORM_SEQ for _, f in seg)
        assert all(ms[i] > 0 for i in range(n))
    finally:
        R.close()


def test_refusals_are_host_side(engine, knobs):
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(10)
    try:
        xs = [rng.randrange(1, c.nsq) for _ in range(6)]
        x = R.up(xs, 2 * c.nw)
        out = ctypes.c_void_p()

        def call(key, xb, ids, groups, n_segments):
            a = np.array(ids, dtype=np.uint32) if ids is not None else None
            return L.pgpu_batch_ct_segment_sum(key, xb, a.ctypes.data_as(ctypes.c_void_p) if a is not None else None,
                                               groups, n_segments, ctypes.byref(out))
        good = [0, 1, 2, 0, NONE, 1]
        assert call(c.pk._h, x, [0, 1, 3, 0, 0, 1], 1, 3) == -1 and b"segment id" in L.pgpu_last_error()   # id out of range
        assert call(c.pk._h, x, [0, 1, 0xFFFFFFFE, 0, 0, 1], 1, 3) == -1
        assert call(c.pk._h, x, good, 0, 3) == -1 and call(c.pk._h, x, good, 1, 0) == -1
        assert call(None, x, good, 1, 3) == -1 and call(c.pk._h, None, good, 1, 3) == -1 and call(c.pk._h, x, None, 1, 3) == -1
        assert L.pgpu_batch_ct_segment_sum(c.pk._h, x, np.array(good, dtype=np.uint32).ctypes.data_as(ctypes.c_void_p), 1, 3, None) == -1
        assert call(c.pk._h, x, good, 1 << 40, 1 << 40) == -1                                   # groups * n_segments overflows
        assert call(c.pk._h, R.up([3, 5], c.nw), [0, 0], 1, 1) == -1 and b"width" in L.pgpu_last_error()
        # a batch of another key: pair rows of a 1024-bit key, and words of the wrong width
        c1 = Case(engine, 1024)
        try:
            x1 = c1.encrypt([1, 2, 3, 4, 5, 6], rng)
            assert call(c.pk._h, x1, good, 1, 3) == -1
            p3, q3, hs3 = key_case(3072, True)
            assert call(engine.PublicKey(p3 * q3, 3072, hs=hs3)._h, x, good, 1, 3) == -1
        finally:
            c1.R.close()
        assert not out.value
        # the masked table-gather policy: refused, and the text says why
        assert L.pgpu_set_table_gather_policy(1) == 0
        try:
            assert call(c.pk._h, x, good, 1, 3) == -3
            assert b"masked" in L.pgpu_last_error() and not out.value
        finally:
            L.pgpu_set_table_gather_policy(0)
        assert R.down(c.segsum(x, good, 1, 3)) == c.expect(xs, good, 1, 3)
        # a key class without pair rows
        p4, q4, _ = key_case(4096, False)
        pk4 = engine.PublicKey(p4 * q4, 4096)
        x4 = R.up([3, 5], 128)
        assert call(pk4._h, x4, [0, 0], 1, 1) == -3 and b"pair" in L.pgpu_last_error() and not out.value
        chunk, levels = ctypes.c_int(), ctypes.c_int()
        assert L.pgpu_ct_segment_sum_plan(4096, 10, 1, 10, ctypes.byref(chunk), ctypes.byref(levels)) == -3
        assert L.pgpu_ct_segment_sum_plan(2048, 10, 0, 10, ctypes.byref(chunk), ctypes.byref(levels)) == -1
    finally:
        R.close()


_NO_PAIR_ROWS = r"""
import ctypes, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
pk = pa.PublicKey(p * q, 2048, hs=hs)
R = Res()
x = R.up([3, 5, 7], 64)
ids = np.array([0, 1, 0], dtype=np.uint32)
out = ctypes.c_void_p()
rc = R.L.pgpu_batch_ct_segment_sum(pk._h, x, ids.ctypes.data_as(ctypes.c_void_p), 1, 2, ctypes.byref(out))
print("rc", rc, R.L.pgpu_last_error().decode())
R.close()
sys.exit(0 if rc == -3 and not out.value else 1)
"""


def test_refused_without_pair_rows(engine):
    """PGPU_PAIR_ROWS=0 keeps resident ciphertexts as Montgomery-form words: no pair form, PGPU_ERR_UNSUPPORTED (own
    process: the switch is read once)"""
    env = dict(os.environ, PGPU_PAIR_ROWS="0")
    r = subprocess.run([sys.executable, "-c", _NO_PAIR_ROWS, ROOT], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


def test_python_segment_sum(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(4)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    m = [rng.randrange(1 << 40) for _ in range(12)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    ids = [0, 1, 2, None, 1, 1, 0, 2, None, 0, 1, 2]
    want = [sum(v for v, s in zip(m, ids) if s == k) % n for k in range(4)]
    assert sk.decrypt(pk.segment_sum(ct, ids, 4)) == want                     # segment 3 is empty: 0
    ids2 = [(s + 1) % 3 if s is not None else None for s in ids]
    got = sk.decrypt(pk.segment_sum(ct, [ids, ids2], 3))                      # two groupings of the same x
    assert got == want[:3] + [sum(v for v, s in zip(m, ids2) if s == k) % n for k in range(3)]
    with pytest.raises(RuntimeError):
        pk.segment_sum(ct, [0, 1, 2], 3)                                      # size mismatch
    with pytest.raises(RuntimeError):
        pk.segment_sum(ct, [3] + [0] * 11, 3)                                 # id out of range
    with pytest.raises(RuntimeError):
        pk.segment_sum(ct, [-1] + [0] * 11, 3)
    with pytest.raises(RuntimeError):
        pk.segment_sum(ct, [0] * 12, 0)
