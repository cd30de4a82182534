"""The encrypted segmented prefix sum on resident ciphertexts (pgpu_batch_ct_segment_scan; csrc/hensel_segscan.hpp) on the
GPU: x read as [rows][seg_len],
    out[r][t] = prod_{ u <= t } x[r][u] mod n^2          (PGPU_SCAN_REVERSE: u >= t)
held bit-identical to Python integers for the 1024-, 2048- and 3072-bit key classes: every shape class (one element, one
row, rows that are no multiple of the chains of a wavefront, rows longer than the chunk), forced chunks that reach three
levels, both directions, edge ciphertexts, inputs in every form a resident ciphertext batch can have, the agreement with
pgpu_batch_ct_segment_sum and with the lower-triangular 0/1 matrix-vector route, the round trip through CRT decrypt, two
lanes at once, the timing record and the refusals.  In the reference such a running sum is composed from
CipherText::operator+ (ipcl/ciphertext.cpp:35-72) element by element."""
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
REVERSE = 1                           # PGPU_SCAN_REVERSE
KIND_SEGSCAN, FORM_SEQ = 7, 2         # PGPU_KERNEL_SEGSCAN, PGPU_FORM_SEQ (include/pgpu.h)
SHAPES = [(1, 1), (1, 2), (3, 7), (5, 32), (17, 5), (1, 65), (2, 300)]       # (rows, seg_len)


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

    def scan(self, x, seg_len, reverse=False):
        return self.R.op(self.L.pgpu_batch_ct_segment_scan, self.pk._h, x, seg_len, REVERSE if reverse else 0)

    def expect(self, xs, seg_len, reverse=False):
        out = [None] * len(xs)
        for r in range(len(xs) // seg_len):
            acc = 1
            for t in (range(seg_len - 1, -1, -1) if reverse else range(seg_len)):
                acc = acc * xs[r * seg_len + t] % self.nsq
                out[r * seg_len + t] = acc
        return out

    def plan(self, rows, seg_len):
        chunk, levels, products = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert self.L.pgpu_ct_segment_scan_plan(self.bits, rows, seg_len, ctypes.byref(chunk), ctypes.byref(levels),
                                                ctypes.byref(products)) == 0
        return chunk.value, levels.value, products.value


@pytest.fixture
def knobs(monkeypatch):
    monkeypatch.delenv("PGPU_SEGSCAN_CHUNK", raising=False)
    monkeypatch.delenv("PGPU_SEGSUM_CHUNK", raising=False)

    def force(c=None):
        if c is None:
            monkeypatch.delenv("PGPU_SEGSCAN_CHUNK", raising=False)
        else:
            monkeypatch.setenv("PGPU_SEGSCAN_CHUNK", str(c))
    return force


def model_levels(chunk, m):
    levels = 1
    while m > chunk:
        m = -(-m // chunk) - 1
        levels += 1
    return levels


@pytest.mark.parametrize("bits", BITS)
def test_segment_scan_is_exact_at_every_shape(engine, knobs, bits):
    """x from a resident DJN encrypt; the chunk the policy picks (one chain per row up to 8 entries, chunks of 8 beyond)"""
    c = Case(engine, bits)
    rng = random.Random(bits)
    L = c.L
    try:
        for rows, seg_len in SHAPES:
            x = c.encrypt([rng.randrange(c.n) for _ in range(rows * seg_len)], rng)
            xs = c.R.down(x)
            for reverse in (False, True):
                y = c.scan(x, seg_len, reverse)
                assert L.pgpu_batch_count(y) == rows * seg_len
                assert L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(x) > 0 and L.pgpu_batch_lane(y) == L.pgpu_batch_lane(x)
                assert c.R.down(y) == c.expect(xs, seg_len, reverse), (rows, seg_len, reverse)
            assert c.R.down(x) == xs                                # the input is left as it was
            c.R.close()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_forced_chunks_reach_three_levels(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    try:
        pool = [rng.randrange(1, c.nsq) for _ in range(3 * 65)]
        for chunk, lens in ((2, (2, 3, 5, 9)), (3, (3, 4, 10, 28)), (8, (8, 9, 65))):
            knobs(chunk)
            for seg_len in lens:
                for rows in (1, 3):
                    got_chunk, got_levels, products = c.plan(rows, seg_len)
                    assert got_chunk == chunk and got_levels == model_levels(chunk, seg_len)
                    if seg_len <= chunk:
                        assert got_levels == 1 and products == rows * (seg_len - 1)
                    xs = pool[:rows * seg_len]
                    x = c.R.up(xs, 2 * c.nw)
                    for reverse in (False, True):
                        assert c.R.down(c.scan(x, seg_len, reverse)) == c.expect(xs, seg_len, reverse), (chunk, seg_len, rows, reverse)
                c.R.close()
        knobs(2)
        assert c.plan(1, 9)[1] == 3 and c.plan(1, 5)[1] == 2        # chunk^3 + 1 entries: three levels
        knobs(8)
        assert c.plan(3, 65) == (8, 2, 3 * (64 + 8 * 7 + 7))
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_edge_values(engine, knobs, bits):
    """the edge ciphertexts of the segmented-sum tests: 1 and n^2 - 1 in runs, at the start and the end of a row"""
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    try:
        xs = [1, c.nsq - 1, 1, c.nsq - 1, c.nsq - 1] + [rng.randrange(1, c.nsq) for _ in range(6)] + [c.nsq - 1]
        x = c.R.up(xs, 2 * c.nw)
        for chunk in (None, 2):
            knobs(chunk)
            for seg_len in (12, 6, 4, 1):
                for reverse in (False, True):
                    assert c.R.down(c.scan(x, seg_len, reverse)) == c.expect(xs, seg_len, reverse), (chunk, seg_len, reverse)
        ones = c.R.up([1] * 10, 2 * c.nw)
        assert c.R.down(c.scan(ones, 5)) == [1] * 10
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_inputs_in_every_form_and_round_trip(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    try:
        rows, seg_len = 3, 11
        m = [rng.randrange(c.n) for _ in range(rows * seg_len)]
        x = c.encrypt(m, rng)                                   # resident DJN encrypt: pair rows
        xs = R.down(x)
        want = c.expect(xs, seg_len)
        y = c.scan(x, seg_len)
        assert R.down(y) == want
        assert R.down(c.scan(R.up(xs, 2 * c.nw), seg_len)) == want                # uploaded plain ciphertext words
        # CRT decrypt of the scan: the cumulative sums of the plaintexts modulo n, both directions
        d = R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, y))
        assert d == [sum(m[r * seg_len:r * seg_len + t + 1]) % c.n for r in range(rows) for t in range(seg_len)]
        d = R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, c.scan(x, seg_len, True)))
        assert d == [sum(m[r * seg_len + t:(r + 1) * seg_len]) % c.n for r in range(rows) for t in range(seg_len)]
        # a scan of a scan (the output of a previous scan as input), across the level boundary too
        knobs(4)
        z = c.scan(y, seg_len, True)
        assert R.down(z) == c.expect(want, seg_len, True)
        knobs(None)
        # the output of pgpu_batch_ct_segment_sum: a histogram [groups][n_segments], scanned along its bins
        groups, n_segments = 2, 5
        ids = [rng.randrange(n_segments) for _ in range(groups * len(m))]
        a = np.array(ids, dtype=np.uint32)
        h = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, x, a.ctypes.data_as(ctypes.c_void_p), groups, n_segments)
        hs = R.down(h)
        for reverse in (False, True):
            assert R.down(c.scan(h, n_segments, reverse)) == c.expect(hs, n_segments, reverse)
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_agrees_with_segment_sum_and_the_matvec_route(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 4)
    L, R = c.L, c.R
    try:
        rows, seg_len = 4, 13
        x = c.encrypt([rng.randrange(c.n) for _ in range(rows * seg_len)], rng)
        a = np.array([j // seg_len for j in range(rows * seg_len)], dtype=np.uint32)
        totals = R.down(R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, x, a.ctypes.data_as(ctypes.c_void_p), 1, rows))
        for chunk in (None, 3):
            knobs(chunk)
            fwd, rev = R.down(c.scan(x, seg_len)), R.down(c.scan(x, seg_len, True))
            assert [fwd[r * seg_len + seg_len - 1] for r in range(rows)] == totals   # the last element of every forward row
            assert [rev[r * seg_len] for r in range(rows)] == totals                 # the first element of every reverse row
        knobs(None)
        # what a caller can do today: one row of 12 through pgpu_batch_ct_matvec with the lower-triangular 0/1 matrix
        x12 = c.encrypt([rng.randrange(c.n) for _ in range(12)], rng)
        w = R.up([1 if j <= i else 0 for i in range(12) for j in range(12)], 1)
        mv = R.down(R.op(L.pgpu_batch_ct_matvec, c.pk._h, x12, w, 12, 1))
        assert R.down(c.scan(x12, 12)) == mv
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
            rng = random.Random(700 + lane)
            rows, seg_len = 2 + lane, 30 + lane                 # beyond the chunk of 8: up-sweep, recursion and down-sweep
            xs = [rng.randrange(1, c.nsq) for _ in range(rows * seg_len)]
            x = R.up(xs, 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for reverse in (False, True):
                y = R.op(L.pgpu_batch_ct_segment_scan, c.pk._h, x, seg_len, REVERSE if reverse else 0)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, reverse)] = (R.down(y), xs, seg_len, reverse)
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
    for got, xs, seg_len, reverse in results.values():
        assert got == c.expect(xs, seg_len, reverse)


def test_launches_carry_the_segscan_kind(engine, knobs):
    c = Case(engine, 2048)
    rng = random.Random(11)
    L, R = c.L, c.R
    try:
        knobs(4)
        x = c.encrypt([rng.randrange(c.n) for _ in range(2 * 21)], rng)   # pair rows already: no conversion launch
        xs = R.down(x)
        chunk, levels, _ = c.plan(2, 21)                                   # chunk 4: 21 -> 5 totals -> 1 total: three levels
        assert (chunk, levels) == (4, 3)
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)                 # drop what earlier calls left
            y = c.scan(x, 21)
            assert L.pgpu_synchronize() == 0
            n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)    # (before the download, which may launch a conversion)
            got = R.down(y)
        finally:
            L.pgpu_set_timing(0)
        assert got == c.expect(xs, 21)
        assert n == 2 * levels - 1                                         # an up-sweep per level but the deepest, a scan per level
        assert all(kinds[i] == KIND_SEGSCAN and forms[i] == FORM_SEQ for i in range(n))   # the segsum_kernel launches too
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

        def call(key, xb, seg_len, flags=0):
            return L.pgpu_batch_ct_segment_scan(key, xb, seg_len, flags, ctypes.byref(out))
        assert call(c.pk._h, x, 0) == -1 and b"seg_len" in L.pgpu_last_error()
        assert call(c.pk._h, x, 4) == -1 and call(c.pk._h, x, 7) == -1             # 6 % seg_len != 0
        assert call(c.pk._h, x, 3, 2) == -1 and b"flag" in L.pgpu_last_error()
        assert call(c.pk._h, x, 3, 3) == -1 and call(c.pk._h, x, 3, 0x80000000) == -1
        assert call(None, x, 3) == -1 and call(c.pk._h, None, 3) == -1
        assert L.pgpu_batch_ct_segment_scan(c.pk._h, x, 3, 0, None) == -1
        assert call(c.pk._h, R.up([3, 5], c.nw), 2) == -1 and b"width" in L.pgpu_last_error()
        # a batch of another key: pair rows of a 1024-bit key, and words of the wrong width
        c1 = Case(engine, 1024)
        try:
            x1 = c1.encrypt([1, 2, 3, 4, 5, 6], rng)
            assert call(c.pk._h, x1, 3) == -1
            p3, q3, hs3 = key_case(3072, True)
            assert call(engine.PublicKey(p3 * q3, 3072, hs=hs3)._h, x, 3) == -1
        finally:
            c1.R.close()
        assert not out.value                                   # (stale handles: test_stale_handles_are_refused, own process)
        # the masked table-gather policy: refused, and the text says why
        assert L.pgpu_set_table_gather_policy(1) == 0
        try:
            assert call(c.pk._h, x, 3) == -3
            assert b"masked" in L.pgpu_last_error() and not out.value
        finally:
            L.pgpu_set_table_gather_policy(0)
        assert R.down(c.scan(x, 3)) == c.expect(xs, 3)
        # a key class without pair rows
        p4, q4, _ = key_case(4096, False)
        pk4 = engine.PublicKey(p4 * q4, 4096)
        x4 = R.up([3, 5], 128)
        assert call(pk4._h, x4, 2) == -3 and b"pair" in L.pgpu_last_error() and not out.value
        chunk, levels, products = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        args = (ctypes.byref(chunk), ctypes.byref(levels), ctypes.byref(products))
        assert L.pgpu_ct_segment_scan_plan(4096, 10, 10, *args) == -3
        assert L.pgpu_ct_segment_scan_plan(2048, 0, 10, *args) == -1 and L.pgpu_ct_segment_scan_plan(2048, 10, 0, *args) == -1
        knobs(2)                                                                   # more chunks than a carry index addresses
        assert L.pgpu_ct_segment_scan_plan(2048, 1, (1 << 32) + 2, *args) == -1 and b"carry" in L.pgpu_last_error()
        assert L.pgpu_ct_segment_scan_plan(2048, 1, 9, None, None, None) == 0
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
rc = R.L.pgpu_batch_ct_segment_scan(pk._h, x, 2, 0, ctypes.byref(out))
print("rc", rc, R.L.pgpu_last_error().decode())
R.close()
sys.exit(0 if rc == -3 and not out.value else 1)
"""


_STALE = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import pailliercryptolib_amd as pa
from test_gpu_pair_rows import Res, key_case
pa.initialize()
p, q, hs = key_case(2048, True)
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
    rc = L.pgpu_batch_ct_segment_scan(key._h, x, 2, 0, ctypes.byref(out))
    print("rc", rc, L.pgpu_last_error().decode())
    ok = ok and rc == -1 and b"shut down" in L.pgpu_last_error() and not out.value
rc = L.pgpu_batch_ct_segment_scan(new_key._h, new_x, 2, 0, ctypes.byref(out))
ok = ok and rc == 0 and bool(out.value)
if out.value:
    got = R.down(out)
    L.pgpu_batch_destroy(out)
    ok = ok and got == [3, 15, 7, 63]
    print("scan", got)
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


def test_python_segment_scan(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(4)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    m = [rng.randrange(1 << 40) for _ in range(12)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    assert sk.decrypt(pk.segment_scan(ct, 4)) == [sum(m[r * 4:r * 4 + t + 1]) for r in range(3) for t in range(4)]
    assert sk.decrypt(pk.segment_scan(ct, 12, reverse=True)) == [sum(m[t:]) for t in range(12)]
    with pytest.raises(RuntimeError):
        pk.segment_scan(ct, 5)                                                # 12 % 5 != 0
    with pytest.raises(RuntimeError):
        pk.segment_scan(ct, 0)
    with pytest.raises(RuntimeError):
        pk.segment_scan([], 1)
