"""Gather, concat and slice of resident batches (pgpu_batch_gather / _concat / _slice; csrc/gather.hpp) on the GPU, through
ctypes, everything resident.  Rows move as bytes, so the expected value of every call is Python list indexing of the
integers that went in (a sentinel reads as 1): pair rows of 1024-, 2048- and 3072-bit keys, the Montgomery words of a
3212-bit key, uploaded ciphertext words, plaintext batches of 1, 3 and 33 words; sources of 1, 5 and 300 rows; outputs of 1,
r - 1, r, r + 1 and one workgroup's rows + 1 for the plan's r rows per wavefront; the reversal, all-equal indices, first and
last row only, random lists with repeats, sentinels at both ends and throughout.  Then what the results feed (CRT decrypt,
segment sum, matmul, weighted sum), several sources, slices, a plan image beyond the bounce buffer, lanes, the timing
record and every refusal.  There are no tolerances.  In the reference the re-ordering calls (CipherText::rotate,
ipcl/ciphertext.cpp:96-104; BaseText::getChunk, base_text.cpp) index host vectors."""
import ctypes
import hashlib
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
KIND_GATHER, FORM_FULL_WIDTH = 15, 0      # PGPU_KERNEL_GATHER, PGPU_FORM_FULL_WIDTH (include/pgpu.h)
ONE = 0xFFFFFFFFFFFFFFFF                  # PGPU_GATHER_ONE
INVALID, UNSUPPORTED = -1, -3
MONT_BITS = 3212                          # tests/golden/key_widths.json: the first width whose results are Montgomery words


class Case:
    """a key of a standard class, and helpers that keep everything resident"""

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


@pytest.fixture(scope="module")
def keys(engine):
    """one key object per width for the whole file"""
    made = {}

    def get(bits):
        if bits not in made:
            if bits == MONT_BITS:
                from test_gpu_key_widths import Key
                made[bits] = Key(engine, bits)
            else:
                made[bits] = Case(engine, bits)
        return made[bits]
    yield get
    for c in made.values():
        c.R.close()


def arr_of(hs):
    return (ctypes.c_void_p * len(hs))(*[h.value for h in hs])


def gather(L, R, hs, idx):
    """one pgpu_batch_gather call; idx: ints, None for the sentinel"""
    ia = np.array([ONE if v is None else v for v in idx], dtype=np.uint64)
    y = R.op(L.pgpu_batch_gather, arr_of(hs), len(hs), ia.ctypes.data_as(ctypes.c_void_p), len(idx))
    ia[:] = 0x7777777777777777                                   # idx is consumed before the call returns
    return y


def concat(L, R, hs):
    return R.op(L.pgpu_batch_concat, arr_of(hs), len(hs))


def take(vals, idx):
    return [1 if i is None else vals[i] for i in idx]


def plan(L, h):
    """(row bytes, lanes per row, rows per wavefront, bytes per access) of a gather from batches like h"""
    row = 4 * L.pgpu_batch_row_limbs(h) or 8 * L.pgpu_batch_words(h)
    a, b, c = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
    assert L.pgpu_batch_gather_plan(row, 1, ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)) == 0
    return row, a.value, b.value, c.value


KINDS = ["pair1024", "pair2048", "pair3072", "mont", "ctwords", "words1", "words3", "words33"]
ROW_BYTES = {"pair1024": 304, "pair2048": 576, "pair3072": 896, "mont": 8 * 102, "ctwords": 512, "words1": 8, "words3": 24,
             "words33": 264}


def make_source(keys, kind, count, rng, R):
    """-> (handle, its values as ints, the plaintexts or None)"""
    if kind.startswith("pair"):
        c = keys(int(kind[4:]))
        m = [rng.randrange(c.n) for _ in range(count)]
        h = c.encrypt(m, rng, R)
        assert c.L.pgpu_batch_row_limbs(h) > 0                   # resident DJN encrypt results: pair rows
        return h, R.down(h), m
    if kind == "mont":
        K = keys(MONT_BITS)
        m = [rng.getrandbits(64 * K.mw) % K.n for _ in range(count)]
        r = [rng.getrandbits(64) for _ in range(count)]
        h = R.op(K.L.pgpu_batch_encrypt, K.pk._h, R.up(m, K.mw), R.up(r, K.rw), 64 * K.rw)
        assert K.L.pgpu_batch_row_limbs(h) == 0 and K.L.pgpu_batch_is_montgomery(h) == 1    # Montgomery words
        return h, R.down(h), m
    if kind == "ctwords":
        c = keys(2048)
        v = [rng.randrange(1, c.nsq) for _ in range(count)]
        return R.up(v, 2 * c.nw), v, None
    words = int(kind[5:])
    v = [rng.getrandbits(64 * words) for _ in range(count)]
    return R.up(v, words), v, None


def index_lists(count, n_out, rng):
    last = count - 1
    some = lambda: rng.randrange(count)                          # noqa: E731
    lists = {
        "reversal": [(last - i) % count for i in range(n_out)],
        "all equal": [count // 2] * n_out,
        "first and last": [0 if i % 2 == 0 else last for i in range(n_out)],
        "random with repeats": [some() for _ in range(n_out)],
        "sentinel first": [None] + [some() for _ in range(n_out - 1)],
        "sentinel last": [some() for _ in range(n_out - 1)] + [None],
        "sentinels throughout": [None if rng.randrange(3) == 0 else some() for _ in range(n_out)],
        "only sentinels": [None] * n_out,
    }
    return lists


@pytest.mark.parametrize("kind", KINDS)
def test_gather_is_list_indexing(engine, keys, kind):
    L = keys(2048).L
    R = Res()
    rng = random.Random(KINDS.index(kind) + 100)
    try:
        for count in (1, 5, 300):
            h, vals, _ = make_source(keys, kind, count, rng, R)
            row, lanes, r, vec = plan(L, h)
            assert row == ROW_BYTES[kind] and vec == (16 if row % 16 == 0 else 8) and lanes * r == 64
            for n_out in sorted({1, r - 1, r, r + 1, 4 * r + 1, count} - {0}):
                for name, idx in index_lists(count, n_out, rng).items():
                    y = gather(L, R, [h], idx)
                    assert L.pgpu_batch_count(y) == n_out and L.pgpu_batch_words(y) == L.pgpu_batch_words(h)
                    assert L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(h)
                    assert L.pgpu_batch_is_montgomery(y) == L.pgpu_batch_is_montgomery(h)
                    assert L.pgpu_batch_lane(y) == L.pgpu_batch_lane(h)
                    assert R.down(y) == take(vals, idx), (count, n_out, name)
                    L.pgpu_batch_destroy(R.live.pop())
            assert R.down(h) == vals                                 # the source is unchanged
    finally:
        R.close()


@pytest.mark.parametrize("bits", [1024, 2048, 3072, MONT_BITS])
def test_gather_then_decrypt(engine, keys, bits):
    """gather then CRT decrypt gives m[idx], 0 at the sentinels; the result feeds CT + CT like any other batch"""
    kind = "mont" if bits == MONT_BITS else "pair%d" % bits
    c = keys(bits)
    L, R = c.L, Res()
    rng = random.Random(bits + 5)
    try:
        h, _, m = make_source(keys, kind, 9, rng, R)
        idx = [None, 8, 0, 3, 3, None, 5, 1, 8, 7, None]
        y = gather(L, R, [h], idx)
        want = [0 if i is None else m[i] for i in idx]
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, y)) == want
        s = R.op(L.pgpu_batch_ct_add, c.pk._h, y, y)
        assert R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, s)) == [2 * v % c.n for v in want]
    finally:
        R.close()


def test_segment_sum_and_matmul_over_a_gather(engine, keys):
    """segment_sum over gather(x, perm) and over an upload of the permuted list, matmul on a gathered minibatch of 3 of 7
    vectors and on the uploaded minibatch: the same bits"""
    c = keys(2048)
    L, R = c.L, Res()
    rng = random.Random(77)
    try:
        count, n_seg = 37, 5
        x, vals, _ = make_source(keys, "pair2048", count, rng, R)
        perm = list(range(count))
        rng.shuffle(perm)
        ids = np.array([rng.randrange(n_seg) for _ in range(count)], dtype=np.uint32)
        idp = ids.ctypes.data_as(ctypes.c_void_p)
        a = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, gather(L, R, [x], perm), idp, 1, n_seg)
        b = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, R.up([vals[i] for i in perm], 2 * c.nw), idp, 1, n_seg)
        want = [1] * n_seg
        for j, i in enumerate(perm):
            want[ids[j]] = want[ids[j]] * vals[i] % c.nsq
        assert R.down(a) == R.down(b) == want
        n_vec, cols, rows, pick = 7, 5, 4, [5, 0, 3]
        xs, xv, _ = make_source(keys, "pair2048", n_vec * cols, rng, R)
        w = [rng.getrandbits(16) for _ in range(rows * cols)]
        wb = R.up(w, 1)
        idx = [v * cols + j for v in pick for j in range(cols)]
        ya = R.op(L.pgpu_batch_ct_matmul, c.pk._h, gather(L, R, [xs], idx), wb, len(pick), rows, 16, 0)
        yb = R.op(L.pgpu_batch_ct_matmul, c.pk._h, R.up([xv[i] for i in idx], 2 * c.nw), wb, len(pick), rows, 16, 0)
        want = []
        for v in pick:
            for i in range(rows):
                acc = 1
                for j in range(cols):
                    acc = acc * pow(xv[v * cols + j], w[i * cols + j], c.nsq) % c.nsq
                want.append(acc)
        assert R.down(ya) == R.down(yb) == want
    finally:
        R.close()


@pytest.mark.parametrize("kind", ["pair2048", "words3", "mont"])
@pytest.mark.parametrize("n_src", [1, 2, 17])
def test_several_sources(engine, keys, kind, n_src):
    """sources of unequal counts: concat is the joined list; gather across them, the same handle named twice, is indexing
    of the joined list"""
    L = keys(2048).L
    R = Res()
    rng = random.Random(n_src * 10 + len(kind))
    try:
        counts = [1 + (7 * k + 3) % 6 for k in range(n_src)]
        made = [make_source(keys, kind, n, rng, R) for n in counts]
        hs, joined = [h for h, _, _ in made], [v for _, vals, _ in made for v in vals]
        y = concat(L, R, hs)
        assert L.pgpu_batch_count(y) == len(joined) and L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(hs[0])
        assert R.down(y) == joined
        hs2, joined2 = hs + [hs[0]], joined + made[0][1]              # the first handle again, at the end
        assert R.down(concat(L, R, hs2)) == joined2
        idx = [len(joined2) - 1, 0, None] + [rng.randrange(len(joined2)) for _ in range(40)] + list(range(len(joined2)))
        assert R.down(gather(L, R, hs2, idx)) == take(joined2, idx)
        for h, vals, _ in made:
            assert R.down(h) == vals
    finally:
        R.close()


def test_segment_sum_over_concat_is_the_plain_weighted_sum(engine, keys):
    """K = 5 clients' encrypt results stacked, id = position: bit-identical to pgpu_batch_ct_weighted_sum(weights = NULL)"""
    c = keys(2048)
    L, R = c.L, Res()
    rng = random.Random(31)
    try:
        K, count = 5, 11
        hs = [make_source(keys, "pair2048", count, rng, R)[0] for _ in range(K)]
        ids = np.array([i for _ in range(K) for i in range(count)], dtype=np.uint32)
        a = R.op(L.pgpu_batch_ct_segment_sum, c.pk._h, concat(L, R, hs), ids.ctypes.data_as(ctypes.c_void_p), 1, count)
        b = R.op(L.pgpu_batch_ct_weighted_sum, c.pk._h, arr_of(hs), K, None, 0)
        xs = [R.down(h) for h in hs]
        want = [1] * count
        for x in xs:
            want = [u * v % c.nsq for u, v in zip(want, x)]
        assert R.down(a) == R.down(b) == want
    finally:
        R.close()


@pytest.mark.parametrize("kind", ["pair1024", "pair2048", "words1", "words33"])
def test_slices(engine, keys, kind):
    L = keys(2048).L
    R = Res()
    rng = random.Random(len(kind) + 40)
    try:
        n_vec, cols = 9, 7
        count = n_vec * cols
        h, vals, _ = make_source(keys, kind, count, rng, R)
        for step in (1, 2, 7):
            for start in (0, 3, count - 1):
                most = (count - 1 - start) // step + 1
                for n in sorted({1, most // 2, most} - {0}):
                    y = R.op(L.pgpu_batch_slice, h, start, n, step)
                    assert L.pgpu_batch_count(y) == n and L.pgpu_batch_row_limbs(y) == L.pgpu_batch_row_limbs(h)
                    assert R.down(y) == [vals[start + i * step] for i in range(n)], (step, start, n)
        for col in (0, cols - 1):                                    # the strided read of [n_vec][cols] as a column
            assert R.down(R.op(L.pgpu_batch_slice, h, col, n_vec, cols)) == vals[col::cols]
        assert R.down(h) == vals
    finally:
        R.close()


def test_plan_image_beyond_the_bounce_buffer(engine, keys):
    """40000 descriptors (320 KB of plan image) over the rows of a 1024-bit key: SHA-256 of the download against the host
    list"""
    c = keys(1024)
    L, R = c.L, Res()
    rng = random.Random(1)
    try:
        count, n_out = 300, 40000
        h, _, _ = make_source(keys, "pair1024", count, rng, R)
        src = np.empty((count, 2 * c.nw), dtype=np.uint64)
        R.check(L.pgpu_batch_download(h, src.ctypes.data_as(ctypes.c_void_p)))
        idx = np.array([rng.randrange(count) for _ in range(n_out)], dtype=np.uint64)
        idx[0], idx[-1], idx[12345] = count - 1, 0, ONE
        y = R.op(L.pgpu_batch_gather, arr_of([h]), 1, idx.ctypes.data_as(ctypes.c_void_p), n_out)
        got = np.empty((n_out, 2 * c.nw), dtype=np.uint64)
        R.check(L.pgpu_batch_download(y, got.ctypes.data_as(ctypes.c_void_p)))
        host = src[np.where(idx == ONE, 0, idx).astype(np.int64)]
        host[12345] = 0
        host[12345, 0] = 1
        assert hashlib.sha256(got.tobytes()).hexdigest() == hashlib.sha256(host.tobytes()).hexdigest()
    finally:
        R.close()


def test_two_lanes_with_a_shared_source(engine, keys):
    """two threads on two batch lanes, each gathering from its own source and from one that lives on a third lane: the
    result sits on the lane of xs[0], the foreign source is ordered in by events"""
    c = keys(2048)
    L = c.L
    results, errors = {}, []
    main = Res()
    R0 = Res()

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            rng = random.Random(900 + lane)
            own, own_vals, _ = make_source(keys, "pair2048", 40, rng, R)
            assert L.pgpu_batch_lane(own) == lane
            for it in range(3):
                idx = [rng.randrange(40 + len(shared_vals)) for _ in range(70)] + [None]
                y = gather(L, R, [own, shared], idx)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = (R.down(y), take(own_vals + shared_vals, idx))
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    try:
        R0.check(L.pgpu_set_batch_lane(3))
        shared, shared_vals, _ = make_source(keys, "pair2048", 50, random.Random(8), R0)
        assert L.pgpu_batch_lane(shared) == 3
        ts = [threading.Thread(target=worker, args=(lane,)) for lane in (1, 2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert len(results) == 6
        for got, want in results.values():
            assert got == want
        assert R0.down(shared) == shared_vals
    finally:
        L.pgpu_set_batch_lane(0)
        R0.close()
        main.close()


def test_timing_record(engine, keys):
    """kind 15, form full-width, one launch for a gather and for a strided slice; concat and the unit-step slice are
    copies and record no kernel"""
    c = keys(2048)
    L, R = c.L, Res()
    rng = random.Random(3)
    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    try:
        h, vals, _ = make_source(keys, "pair2048", 30, rng, R)
        g, gv, _ = make_source(keys, "pair2048", 4, rng, R)
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)               # drop what earlier calls left
            calls = [
                (lambda: gather(L, R, [h, g], [33, 0, None, 29]), 1, [gv[3], vals[0], 1, vals[29]]),
                (lambda: R.op(L.pgpu_batch_slice, h, 1, 5, 6), 1, vals[1::6][:5]),
                (lambda: concat(L, R, [h, g, h]), 0, vals + gv + vals),
                (lambda: R.op(L.pgpu_batch_slice, h, 7, 20, 1), 0, vals[7:27]),
            ]
            for call, launches, want in calls:
                y = call()
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)       # (before the download, which launches a conversion)
                assert n == launches
                assert all(kinds[i] == KIND_GATHER and forms[i] == FORM_FULL_WIDTH and ms[i] > 0 for i in range(n))
                assert R.down(y) == want
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_refusals_are_host_side_and_launch_nothing(engine, keys):
    """every refusal of the three calls that one session on one GPU can provoke (stale handles and pools of more than one
    GPU: test_stale_handles_and_pools_are_refused; a source of 2^32 - 1 rows or more would be 34 GB of one-word rows and is
    NOT provoked here: the rule the calls apply, policy.cpp's gather_counts_ok, is checked on the host by
    tests/cpp/gather_policy_tests.cpp, the refusal that index_admit makes of it is untested); after each one the timing
    record is empty and *out is still null.  The masked table-gather policy does NOT refuse these calls"""
    c, c1 = keys(2048), keys(1024)
    L, R = c.L, Res()
    rng = random.Random(11)
    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    try:
        xp, xpv, _ = make_source(keys, "pair2048", 6, rng, R)
        xq, _, _ = make_source(keys, "pair2048", 4, rng, R)
        x1, _, _ = make_source(keys, "pair1024", 6, rng, R)              # pair rows of another key
        xw, _, _ = make_source(keys, "ctwords", 6, rng, R)               # the same width, plain words
        xm = R.op(L.pgpu_batch_ct_add, keys(MONT_BITS).pk._h, *[make_source(keys, "mont", 3, rng, R)[0]] * 2)   # Montgomery words
        p3, p1 = R.up([1, 2, 3], 3), R.up([1, 2, 3], 1)
        p102 = R.up([1, 2, 3], 102)                                      # as wide as xm, plain
        out = ctypes.c_void_p()
        outp = ctypes.byref(out)
        idx = np.array([0, 1, 2], dtype=np.uint64)
        ip = idx.ctypes.data_as(ctypes.c_void_p)

        def sources(hs):
            return (ctypes.c_void_p * max(1, len(hs)))(*[h.value if h is not None else None for h in hs])

        def bad_index(vals):
            a = np.array(vals, dtype=np.uint64)
            return L.pgpu_batch_gather(sources([xp, xq]), 2, a.ctypes.data_as(ctypes.c_void_p), len(vals), outp)
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)               # drop what earlier calls left
            refused = [
                # null handles, a null out, a null index list
                lambda: L.pgpu_batch_gather(None, 1, ip, 3, outp), lambda: L.pgpu_batch_gather(sources([xp, None]), 2, ip, 3, outp),
                lambda: L.pgpu_batch_gather(sources([xp]), 1, ip, 3, None), lambda: L.pgpu_batch_gather(sources([xp]), 1, None, 3, outp),
                lambda: L.pgpu_batch_concat(None, 1, outp), lambda: L.pgpu_batch_concat(sources([None]), 1, outp),
                lambda: L.pgpu_batch_concat(sources([xp]), 1, None),
                lambda: L.pgpu_batch_slice(None, 0, 1, 1, outp), lambda: L.pgpu_batch_slice(xp, 0, 1, 1, None),
                # n_src == 0 or above 65535, n_out == 0
                lambda: L.pgpu_batch_gather(sources([xp]), 0, ip, 3, outp), lambda: L.pgpu_batch_gather(sources([xp]), 65536, ip, 3, outp),
                lambda: L.pgpu_batch_concat(sources([xp]), 0, outp), lambda: L.pgpu_batch_concat(sources([xp]), 65536, outp),
                lambda: L.pgpu_batch_gather(sources([xp]), 1, ip, 0, outp),
                # an index at or beyond the total count that is not the sentinel
                lambda: bad_index([0, 10, 3]), lambda: bad_index([9, ONE, ONE - 1]), lambda: bad_index([1 << 32]),
                # step == 0, count == 0, slices that run past the end
                lambda: L.pgpu_batch_slice(xp, 0, 3, 0, outp), lambda: L.pgpu_batch_slice(xp, 0, 0, 1, outp),
                lambda: L.pgpu_batch_slice(xp, 6, 1, 1, outp), lambda: L.pgpu_batch_slice(xp, 0, 7, 1, outp),
                lambda: L.pgpu_batch_slice(xp, 1, 4, 2, outp), lambda: L.pgpu_batch_slice(xp, 5, 2, 1 << 63, outp),
                lambda: L.pgpu_batch_slice(xp, ONE, 1, 1, outp), lambda: L.pgpu_batch_slice(xp, 0, ONE, 2, outp),
                # layouts that differ: another key, plain words beside pair rows, other widths, plain beside Montgomery words
                lambda: L.pgpu_batch_gather(sources([xp, x1]), 2, ip, 3, outp), lambda: L.pgpu_batch_concat(sources([xp, xw]), 2, outp),
                lambda: L.pgpu_batch_concat(sources([xw, xp]), 2, outp), lambda: L.pgpu_batch_gather(sources([p3, p1]), 2, ip, 3, outp),
                lambda: L.pgpu_batch_concat(sources([xm, p102]), 2, outp), lambda: L.pgpu_batch_concat(sources([p102, xm]), 2, outp),
            ]
            for i, call in enumerate(refused):
                assert call() == INVALID, i
                assert not out.value, i
            assert bad_index([0, 10, 3, 11]) == INVALID and b"position 1" in L.pgpu_last_error()     # the FIRST offending position
            assert bad_index([0, 9, 3, 10]) == INVALID and b"position 3" in L.pgpu_last_error()
            assert L.pgpu_batch_concat(sources([xp, xw]), 2, outp) == INVALID and b"layout" in L.pgpu_last_error()
            assert L.pgpu_batch_gather_plan(12, 1, None, None, None) == INVALID
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0 and not out.value     # nothing was launched
            # the masked table-gather policy: the address stream depends on the caller's plaintext indices only
            assert L.pgpu_set_table_gather_policy(1) == 0
            try:
                assert R.down(gather(L, R, [xp], [5, None, 0])) == [xpv[5], 1, xpv[0]]
                assert R.down(concat(L, R, [xp, xp])) == xpv + xpv
                assert R.down(R.op(L.pgpu_batch_slice, xp, 1, 2, 3)) == [xpv[1], xpv[4]]
            finally:
                L.pgpu_set_table_gather_policy(0)
        finally:
            L.pgpu_set_timing(0)
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
    finally:
        R.close()


_STALE_AND_POOL = r"""
import ctypes, sys
sys.path.insert(0, sys.argv[1])
sys.path.insert(0, sys.argv[1] + "/tests")
import numpy as np
import pailliercryptolib_amd as pa
from pailliercryptolib_amd import _capi
from test_gpu_pair_rows import Res
pa.initialize()
R = Res()
L = R.L
vals = list(range(3, 35))
old_x = R.up(vals, 2)
L.pgpu_shutdown()                      # the pool the batch was created under is gone
pa.initialize()
new_x = R.up(vals, 2)
out = ctypes.c_void_p()
idx = np.array([1, 0], dtype=np.uint64)
ip = idx.ctypes.data_as(ctypes.c_void_p)
ok = True
def refused(rc, code, text):
    print("rc", rc, L.pgpu_last_error().decode())
    return rc == code and text in L.pgpu_last_error() and not out.value
for hs in ([old_x], [new_x, old_x]):
    arr = (ctypes.c_void_p * len(hs))(*[h.value for h in hs])
    ok = ok and refused(L.pgpu_batch_gather(arr, len(hs), ip, 2, ctypes.byref(out)), -1, b"shut down")
    ok = ok and refused(L.pgpu_batch_concat(arr, len(hs), ctypes.byref(out)), -1, b"shut down")
ok = ok and refused(L.pgpu_batch_slice(old_x, 0, 2, 2, ctypes.byref(out)), -1, b"shut down")
arr = (ctypes.c_void_p * 1)(new_x.value)
rc = L.pgpu_batch_gather(arr, 1, ip, 2, ctypes.byref(out))
ok = ok and rc == 0 and R.down(out) == [vals[1], vals[0]]
L.pgpu_batch_destroy(out)
L.pgpu_batch_destroy(new_x)
out = ctypes.c_void_p()
L.pgpu_shutdown()
_capi.check(L.pgpu_init_all(2))        # two pool entries (on one physical GPU): rows are sharded
ok = ok and L.pgpu_pool_size() == 2
x2 = R.up(vals, 2)
arr = (ctypes.c_void_p * 1)(x2.value)
ok = ok and refused(L.pgpu_batch_gather(arr, 1, ip, 2, ctypes.byref(out)), -3, b"more than one GPU")
ok = ok and refused(L.pgpu_batch_concat(arr, 1, ctypes.byref(out)), -3, b"more than one GPU")
ok = ok and refused(L.pgpu_batch_slice(x2, 0, 2, 2, ctypes.byref(out)), -3, b"more than one GPU")
ok = ok and refused(L.pgpu_batch_slice(x2, 0, 2, 1, ctypes.byref(out)), -3, b"more than one GPU")
ok = ok and R.down(x2) == vals
L.pgpu_batch_destroy(x2)
print("ok", ok)
sys.exit(0 if ok else 1)
"""


def test_stale_handles_and_pools_are_refused(engine):
    """a batch created under a device pool that has been shut down: PGPU_ERR_INVALID_PARAM; a pool of two entries:
    PGPU_ERR_UNSUPPORTED; *out untouched (own process: the pool of the test session stays up)"""
    env = dict(os.environ, PGPU_POOL_OVERSUBSCRIBE="1", PGPU_MIN_SHARD="8")
    r = subprocess.run([sys.executable, "-c", _STALE_AND_POOL, ROOT], capture_output=True, text=True, env=env, timeout=300)
    print(r.stdout[-2000:], r.stderr[-2000:])
    assert r.returncode == 0


def test_python_gather_and_concat(engine):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(6)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    ms = [[rng.randrange(1 << 40) for _ in range(k)] for k in (6, 1, 4)]
    cts = [pk.encrypt(m, [rng.getrandbits(1024) for _ in m]) for m in ms]
    idx = [5, None, 0, 0, 3]
    got = pk.gather(cts[0], idx)
    assert got == [1 if i is None else cts[0][i] for i in idx]
    assert sk.decrypt(got) == [0 if i is None else ms[0][i] for i in idx]
    flat_c, flat_m = [v for c in cts for v in c], [v for m in ms for v in m]
    assert pk.concat(cts) == flat_c
    idx = [10, 6, None, 0]
    assert sk.decrypt(pk.gather(cts, idx)) == [0 if i is None else flat_m[i] for i in idx]
    for bad in ((cts[0], []), ([], [0]), (cts[0], [6]), (cts[0], [-1]), (cts, [11])):
        with pytest.raises(RuntimeError):
            pk.gather(*bad)
    for bad in ([], [cts[0], []]):
        with pytest.raises(RuntimeError):
            pk.concat(bad)
