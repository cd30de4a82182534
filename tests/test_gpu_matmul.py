"""The encrypted matrix product on resident ciphertexts (pgpu_batch_ct_matmul; csrc/hensel_matmul.hpp) on the GPU:
    default      out[v*rows + i] = prod_j x[v*cols + j]^w[i][j] mod n^2
    transposed   out[i*n_vec + v] = prod_j x[j*n_vec + v]^w[i][j] mod n^2
held bit-identical to Python's pow for the 1024-, 2048- and 3072-bit key classes (32 / 16 / 8 groups per wavefront).  The
shapes are the smallest at which the mapping can still go wrong: (3,5,7) has 15 outputs -- one wavefront straddles vectors
and ends in dead groups --, (7,1,9) one row, (2,17,1) one column, (40,3,4) more outputs than one wavefront for every class;
(5,13,33) under forced windows, slices (5 does not divide 33) and tiles (2: a short last pass; in the transposed layout
the staged passes).  Every reference is computed once per shape and shared by both layouts: the transposed call sees the
same matrix of ciphertexts stored the other way round.  Further: edge weights, inputs in every form, two layers chained
through CRT decrypt, the agreement with pgpu_batch_ct_matvec (n_vec = 1) and with the pgpu_batch_ct_spmv formulation on
the same resident x, a call whose short last pass runs on more slices than its full passes, two lanes at once, the
refusals, the timing record and the Python layer.
(One refusal of the header cannot be reached through the C-ABI: n_vec * rows beyond size_t needs n_vec <= count(x) and
rows <= count(w) whose product overflows -- more elements than two batches can hold.)"""
import ctypes
import json
import os
import random
import subprocess
import sys
import threading

import numpy as np
import pytest

from test_gpu_matvec import Case, rand_weights
from test_gpu_pair_rows import Res, key_case  # noqa: F401 -- (Res: the child processes below name it too)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = [1024, 2048, 3072]
SHAPES = [(1, 1, 1), (1, 5, 33), (3, 5, 7), (7, 1, 9), (2, 17, 1), (5, 13, 33), (40, 3, 4)]
KNOBS = ("PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES")
KIND_MATMUL = 11
TRANSPOSED = 1


@pytest.fixture
def knobs(monkeypatch):
    for name in KNOBS + ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_SPMV_WINDOW", "PGPU_SPMV_CHUNK"):
        monkeypatch.delenv(name, raising=False)

    def force(w=None, t=None, s=None):
        for name, v in zip(KNOBS, (w, t, s)):
            if v is None:
                monkeypatch.delenv(name, raising=False)
            else:
                monkeypatch.setenv(name, str(v))
    return force


def matmul(c, x, wb, n_vec, rows, e_bits, flags=0):
    return c.R.op(c.L.pgpu_batch_ct_matmul, c.pk._h, x, wb, n_vec, rows, e_bits, flags)


def expect(c, xs, wm, n_vec):
    """default layout, from the flat [n_vec][cols] values"""
    cols = len(xs) // n_vec
    return [v for k in range(n_vec) for v in c.expect(xs[k * cols:(k + 1) * cols], wm)]


def transpose(flat, outer, inner):
    """[outer][inner] -> [inner][outer]"""
    return [flat[a * inner + b] for b in range(inner) for a in range(outer)]


def both_layouts(c, x, xs, wb, n_vec, rows, e_bits, want, tag):
    """the default call on the resident x, the transposed call on the same matrix of ciphertexts stored [cols][n_vec]"""
    cols = len(xs) // n_vec
    y = matmul(c, x, wb, n_vec, rows, e_bits)
    assert c.L.pgpu_batch_count(y) == n_vec * rows and c.L.pgpu_batch_row_limbs(y) > 0
    assert c.R.down(y) == want, tag
    xt = c.R.up(transpose(xs, n_vec, cols), 2 * c.nw)
    yt = matmul(c, xt, wb, n_vec, rows, e_bits, TRANSPOSED)
    assert c.R.down(yt) == transpose(want, n_vec, rows), tag + ("transposed",)


@pytest.mark.parametrize("bits", BITS)
def test_matmul_is_exact_at_every_shape(engine, knobs, bits):
    """x from a resident DJN encrypt; the plan the policy picks; n_vec = 1 downloads what the matvec downloads"""
    c = Case(engine, bits)
    rng = random.Random(bits)
    try:
        for n_vec, rows, cols in SHAPES:
            e_bits = 32 if n_vec * rows * cols < 1000 else 13
            x = c.encrypt([rng.randrange(c.n) for _ in range(n_vec * cols)], rng)
            xs = c.R.down(x)
            wm = rand_weights(rng, rows, cols, e_bits)
            wb = c.weights(wm, e_bits)
            want = expect(c, xs, wm, n_vec)
            both_layouts(c, x, xs, wb, n_vec, rows, e_bits, want, (n_vec, rows, cols))
            if n_vec == 1:
                mv = c.R.down(c.R.op(c.L.pgpu_batch_ct_matvec, c.pk._h, x, wb, rows, e_bits))
                assert mv == want
                assert c.R.down(matmul(c, x, wb, 1, rows, e_bits, TRANSPOSED)) == mv      # the same handles, both layouts
            c.R.close()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("e_bits", [13, 32])
def test_forced_windows_slices_and_tiles(engine, knobs, bits, e_bits):
    c = Case(engine, bits)
    rng = random.Random(bits + e_bits)
    n_vec, rows, cols = 5, 13, 33
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(n_vec * cols)], rng)
        xs = c.R.down(x)
        wm = rand_weights(rng, rows, cols, e_bits)
        wb = c.weights(wm, e_bits)
        want = expect(c, xs, wm, n_vec)
        for w in (1, 4, 6):
            for s in (1, 2, 5, 33):                       # 5 does not divide 33
                for t in (1, 2, 5):                       # 2: passes of 2, 2 and 1 vectors
                    knobs(w, t, s)
                    assert c.R.down(matmul(c, x, wb, n_vec, rows, e_bits)) == want, (w, s, t)
                c.R.close()
                x = c.R.up(xs, 2 * c.nw)
                wb = c.weights(wm, e_bits)
        knobs(4, 2, 5)
        both_layouts(c, x, xs, wb, n_vec, rows, e_bits, want, ("w4 S5 t2",))
        knobs(6, 2, 1)                                    # the transposed layout, tiled, one slice: stored through the strides
        both_layouts(c, x, xs, wb, n_vec, rows, e_bits, want, ("w6 S1 t2",))
        knobs()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_weight_edge_cases(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    n_vec, cols = 3, 9
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(n_vec * cols)], rng)
        xs = c.R.down(x)
        for e_bits in (1, 32, 64, 127):
            top = (1 << e_bits) - 1
            wm = [[0] * cols,                                                      # all zero: 1 for every vector
                  [1] * cols,
                  [top] * cols,
                  [rng.getrandbits(e_bits) if j % 3 else 0 for j in range(cols)],  # zeros scattered
                  [rng.getrandbits(e_bits) for _ in range(cols)]]
            want = expect(c, xs, wm, n_vec)
            assert all(want[v * len(wm)] == 1 for v in range(n_vec))
            both_layouts(c, x, xs, c.weights(wm, e_bits), n_vec, len(wm), e_bits, want, (e_bits,))
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_input_forms_and_two_layers(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 3)
    L, R = c.L, c.R
    n_vec, cols, r1, r2, e_bits = 4, 11, 6, 3, 20
    try:
        m = [rng.randrange(c.n) for _ in range(n_vec * cols)]
        x = c.encrypt(m, rng)                                       # resident DJN encrypt: pair rows
        xs = R.down(x)
        w1, w2 = rand_weights(rng, r1, cols, e_bits), rand_weights(rng, r2, r1, e_bits)
        want = expect(c, xs, w1, n_vec)
        y = matmul(c, x, c.weights(w1, e_bits), n_vec, r1, e_bits)
        assert R.down(y) == want
        assert R.down(x) == xs                                      # x is left unchanged
        assert R.down(matmul(c, R.up(xs, 2 * c.nw), c.weights(w1, e_bits), n_vec, r1, e_bits)) == want      # plain ciphertext words
        z = matmul(c, y, c.weights(w2, e_bits), n_vec, r2, e_bits)  # a second layer on the first one's result
        assert R.down(z) == expect(c, want, w2, n_vec)
        d = R.down(R.op(L.pgpu_batch_decrypt_crt, c.sk._h, z))
        for v in range(n_vec):
            h = [sum(a * b for a, b in zip(row, m[v * cols:(v + 1) * cols])) for row in w1]
            assert d[v * r2:(v + 1) * r2] == [sum(a * b for a, b in zip(row, h)) % c.n for row in w2]
        # the transposed layers: Y = W1 * X, Z = W2 * Y on [cols][n_vec] storage
        xt = R.up(transpose(xs, n_vec, cols), 2 * c.nw)
        yt = matmul(c, xt, c.weights(w1, e_bits), n_vec, r1, e_bits, TRANSPOSED)
        zt = matmul(c, yt, c.weights(w2, e_bits), n_vec, r2, e_bits, TRANSPOSED)
        assert R.down(zt) == transpose(R.down(z), n_vec, r2)
    finally:
        R.close()


@pytest.mark.parametrize("bits", BITS)
def test_equals_the_spmv_formulation(engine, knobs, bits):
    """the flat matrix as x, n_vec * rows CSR rows of cols entries, column numbers v * cols + j, the weights replicated"""
    c = Case(engine, bits)
    rng = random.Random(bits + 4)
    L, R = c.L, c.R
    n_vec, rows, cols, e_bits = 6, 7, 10, 32
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(n_vec * cols)], rng)
        wm = rand_weights(rng, rows, cols, e_bits)
        flat = [v for row in wm for v in row]
        rp = np.arange(n_vec * rows + 1, dtype=np.uint64) * cols
        ci = np.array([v * cols + j for v in range(n_vec) for _ in range(rows) for j in range(cols)], dtype=np.uint32)
        sp = R.op(L.pgpu_batch_ct_spmv, c.pk._h, x, rp.ctypes.data_as(ctypes.c_void_p), ci.ctypes.data_as(ctypes.c_void_p),
                  R.up(flat * n_vec, 1), n_vec * rows, e_bits)
        for t in (None, 4):
            knobs(None, t, None)
            assert R.down(matmul(c, x, R.up(flat, 1), n_vec, rows, e_bits)) == R.down(sp)
        knobs()
    finally:
        R.close()


@pytest.mark.parametrize("bits,n_vec,tile,rows,cols,s_full,s_last", [(3072, 9, 8, 512, 16, 2, 4), (2048, 9, 8, 512, 32, 4, 8),
                                                                     (3072, 5, 3, 560, 32, 5, 8)])
def test_last_pass_on_more_slices_than_a_full_pass(engine, knobs, bits, n_vec, tile, rows, cols, s_full, s_last):
    """no forced slices: the short last pass runs on its own slice count (plan.last_slices) inside a partial block sized by
    the larger of the two.  9 vectors in tiles of 8 at 3072 bits: a full pass has 4096 outputs = 512 wavefronts, fill 2 under
    the cap 16 / 4; the last pass of one vector 64 wavefronts, fill 16: four slices.  At 2048 bits: 256 and 32 wavefronts,
    four and eight slices of 32 columns -- the fold picks its (4,18) / (8,9) form at two counts within one call.  5 vectors
    in tiles of 3, 70 wavefronts per vector: five slices of three vectors, then eight of two -- the short pass fills MORE of
    the partial block than a full one.  The query of the call itself reports the full passes' count; the two counts are
    read off queries at n_vec = tile and at the vectors of the last pass.  Weights of 2 bits keep Python's reference at
    some 10^5 products"""
    c = Case(engine, bits)
    rng = random.Random(bits + 5)
    e_bits, last = 2, n_vec % tile
    ps, pt = ctypes.c_int(), ctypes.c_size_t()

    def plan(k):
        assert c.L.pgpu_ct_matmul_plan(bits, k, rows, cols, e_bits, None, ctypes.byref(ps), ctypes.byref(pt), None, None) == 0
        return ps.value, pt.value
    try:
        knobs(None, tile, None)
        full, one, whole = plan(tile), plan(last), plan(n_vec)
        print(f"matmul plan, {bits} bits, tile {tile}: slices {full[0]} at n_vec = {tile}, {one[0]} at n_vec = {last}, {whole[0]} at n_vec = {n_vec}")
        assert full == (s_full, tile) and one == (s_last, last) and whole == (s_full, tile)
        xs = [rng.randrange(1, c.nsq) for _ in range(n_vec * cols)]
        wm = rand_weights(rng, rows, cols, e_bits)
        tab = [[pow(x, e, c.nsq) for e in range(4)] for x in xs]         # the weights are below 4: pow once per (x, weight)
        want = []
        for v in range(n_vec):
            for row in wm:
                acc = 1
                for j, e in enumerate(row):
                    if e:
                        acc = acc * tab[v * cols + j][e] % c.nsq
                want.append(acc)
        both_layouts(c, c.R.up(xs, 2 * c.nw), xs, c.weights(wm, e_bits), n_vec, rows, e_bits, want, (bits,))
    finally:
        c.R.close()


def test_two_lanes_at_once(engine, knobs):
    """two threads on different batch lanes, each with its own x, the matrices uploaded by the main thread on its lane: the
    default layout beside the transposed one, both in tiles of 2 over 3 slices (the transposed passes staged and copied
    back); three calls in a row per thread, so that the blocks of one lane come and go while the other's kernels run"""
    c = Case(engine, 2048)
    L = c.L
    rng = random.Random(12)
    results, errors = {}, []
    shapes = {1: (5, 6, 9), 2: (5, 5, 7)}                  # lane: n_vec, rows, cols; lane 2 stores x [cols][n_vec]
    wms = {lane: rand_weights(rng, rows, cols, 32) for lane, (_, rows, cols) in shapes.items()}
    xss = {lane: [rng.randrange(1, c.nsq) for _ in range(n_vec * cols)] for lane, (n_vec, _, cols) in shapes.items()}
    knobs(None, 2, 3)

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            n_vec, rows, cols = shapes[lane]
            x = R.up(xss[lane], 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for it in range(3):
                y = R.op(L.pgpu_batch_ct_matmul, c.pk._h, x, ws[lane], n_vec, rows, 32, TRANSPOSED if lane == 2 else 0)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = R.down(y)
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    try:
        ws = {lane: c.weights(wms[lane], 32) for lane in shapes}     # lane of the main thread: ordered in by events
        ts = [threading.Thread(target=worker, args=(lane,)) for lane in (1, 2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert len(results) == 6
        want1 = expect(c, xss[1], wms[1], 5)
        want2 = transpose(expect(c, transpose(xss[2], 7, 5), wms[2], 5), 5, 5)
        for it in range(3):
            assert results[(1, it)] == want1, it
            assert results[(2, it)] == want2, it
    finally:
        c.R.close()


def test_refusals_are_host_side(engine, knobs):
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(9)
    kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
    try:
        xs = [rng.randrange(1, c.nsq) for _ in range(6)]
        x = R.up(xs, 2 * c.nw)
        xp = c.encrypt([1, 2, 3, 4, 5, 6], rng)
        wm = rand_weights(rng, 2, 3, 32)
        wb = c.weights(wm, 32)                                     # 2 rows x 3 columns: n_vec = 2
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

        def call(*a):
            return L.pgpu_batch_ct_matmul(*a, ctypes.byref(out))
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)         # drop what the set-up left
            invalid = [
                ((None, x, wb, 2, 2, 32, 0), b"null"), ((k, None, wb, 2, 2, 32, 0), b"null"), ((k, x, None, 2, 2, 32, 0), b"null"),
                ((k, x, wb, 0, 2, 32, 0), b"n_vec and rows must be positive"), ((k, x, wb, 2, 0, 32, 0), b"n_vec and rows must be positive"),
                ((k, x, wb, 4, 2, 32, 0), b"n_vec must divide count(x)"),
                ((k, x, wb, 2, 3, 32, 0), b"Size mismatch"), ((k, x, wb, 3, 2, 32, 0), b"Size mismatch"),      # count(w) != rows * cols
                ((k, x, xp, 1, 1, 32, 0), b"plain uploaded batch"),                                           # w in pair rows
                ((k, x, wb, 2, 2, 0, 0), b"e_bits"), ((k, x, wb, 2, 2, 65, 0), b"e_bits"),
                ((k, x, wb, 2, 2, 32, 2), b"unknown flag bit"), ((k, x, wb, 2, 2, 32, 3), b"unknown flag bit"),
                ((k, wide, wb, 2, 2, 32, 0), b"ciphertext width mismatch"),
                ((k, pair_other, wb, 2, 2, 32, 0), b"different key"), ((k, mont_other, wb, 2, 2, 32, 0), b"different key")]
            for args, text in invalid:
                assert call(*args) == -1, args
                assert text in L.pgpu_last_error() and not out.value, (args, L.pgpu_last_error())
            assert L.pgpu_batch_ct_matmul(k, x, wb, 2, 2, 32, 0, None) == -1 and b"null" in L.pgpu_last_error()
            # the masked table-gather policy: refused, and the text says why
            assert L.pgpu_set_table_gather_policy(1) == 0
            try:
                assert call(k, x, wb, 2, 2, 32, 0) == -3
                err = L.pgpu_last_error()
                assert b"matmul" in err and b"masked" in err and b"digits of the plaintext matrix" in err and not out.value
            finally:
                L.pgpu_set_table_gather_policy(0)
            # a key class without pair rows
            p4, q4, _ = key_case(4096, False)
            pk4 = engine.PublicKey(p4 * q4, 4096)
            assert call(pk4._h, R.up([3, 5], 128), R.up([1, 2], 1), 1, 1, 32, 0) == -3 and b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0    # nothing was launched
        finally:
            L.pgpu_set_timing(0)
        assert R.down(matmul(c, x, wb, 2, 2, 32)) == expect(c, xs, wm, 2)
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
x, w = R.up([3, 5, 7, 9], 64), R.up([1, 2], 1)
out = ctypes.c_void_p()
rc = R.L.pgpu_batch_ct_matmul(pk._h, x, w, 2, 1, 32, 0, ctypes.byref(out))
err = R.L.pgpu_last_error()
print("rc", rc, err.decode())
R.close()
sys.exit(0 if rc == -3 and b"matmul: key has no pair form" in err and not out.value else 1)
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
old_x, old_w = R.up([3, 5, 7, 9], 64), R.up([2, 3], 1)
L.pgpu_shutdown()                      # the pool the key and the batches were created under is gone
pa.initialize()
new_key = pa.PublicKey(p * q, 2048, hs=hs)
new_x, new_w = R.up([3, 5, 7, 9], 64), R.up([2, 3], 1)
out = ctypes.c_void_p()
ok = True
for key, x, w in ((old_key, new_x, new_w), (new_key, old_x, new_w), (new_key, new_x, old_w)):
    rc = L.pgpu_batch_ct_matmul(key._h, x, w, 2, 1, 2, 0, ctypes.byref(out))
    print("rc", rc, L.pgpu_last_error().decode())
    ok = ok and rc == -1 and b"shut down" in L.pgpu_last_error() and not out.value
rc = L.pgpu_batch_ct_matmul(new_key._h, new_x, new_w, 2, 1, 2, 0, ctypes.byref(out))
ok = ok and rc == 0 and bool(out.value)
if out.value:
    got = R.down(out)
    L.pgpu_batch_destroy(out)
    ok = ok and got == [3 ** 2 * 5 ** 3 % nsq, 7 ** 2 * 9 ** 3 % nsq]
    print("matmul", got)
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
    """every launch of a call is kind 11; passes * (table build + multi-exponentiation + fold launches) of them, for the plan
    pgpu_ct_matmul_plan reports (the shapes keep the slices of a short last pass those of a full one)"""
    c = Case(engine, 2048)
    L, R = c.L, c.R
    rng = random.Random(31)
    n_vec, rows, cols, e_bits = 5, 3, 20, 16
    try:
        x = c.encrypt([rng.randrange(c.n) for _ in range(n_vec * cols)], rng)     # pair rows already: no conversion launch
        xs = R.down(x)
        wm = rand_weights(rng, rows, cols, e_bits)
        wb = c.weights(wm, e_bits)
        want = expect(c, xs, wm, n_vec)
        xt = R.up(transpose(xs, n_vec, cols), 2 * c.nw)
        xt = R.op(L.pgpu_batch_ct_add, c.pk._h, xt, R.up([1] * (n_vec * cols), 2 * c.nw))      # times 1: the same values as pair rows
        assert L.pgpu_batch_row_limbs(xt) > 0
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        pw, ps, pt, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert L.pgpu_set_timing(1) == 0
        try:
            for forced in ((None, None, None), (None, 2, None), (4, 2, 5), (4, 1, 1), (6, 5, 20)):
                knobs(*forced)
                assert L.pgpu_ct_matmul_plan(2048, n_vec, rows, cols, e_bits, ctypes.byref(pw), ctypes.byref(ps), ctypes.byref(pt),
                                             ctypes.byref(tb), ctypes.byref(pr)) == 0
                passes = -(-n_vec // pt.value)
                launches = passes * (2 + fold_launches(ps.value))
                assert launches <= 64
                for flags, xb, exp in ((0, x, want), (TRANSPOSED, xt, transpose(want, n_vec, rows))):
                    assert L.pgpu_synchronize() == 0
                    L.pgpu_timing_collect_ex(kinds, forms, ms, 64)            # drop what earlier calls left
                    y = matmul(c, xb, wb, n_vec, rows, e_bits, flags)
                    assert L.pgpu_synchronize() == 0
                    n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)        # (before the download, which launches a conversion)
                    assert n == launches, (forced, flags, n, launches)
                    assert all(kinds[i] == KIND_MATMUL and ms[i] > 0 for i in range(n))
                    assert R.down(y) == exp
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


def test_python_matmul(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    rng = random.Random(3)
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    n_vec, cols, rows = 3, 5, 4
    m = [[rng.randrange(1 << 40) for _ in range(cols)] for _ in range(n_vec)]
    flat = [v for r in m for v in r]
    ct = pk.encrypt(flat, [rng.getrandbits(1024) for _ in flat])
    x = [ct[v * cols:(v + 1) * cols] for v in range(n_vec)]
    wm = [[rng.getrandbits(20) for _ in range(cols)] for _ in range(rows)]
    want = [[sum(a * b for a, b in zip(row, m[v])) % n for row in wm] for v in range(n_vec)]
    y = pk.matmul(x, wm)
    assert len(y) == n_vec and all(len(r) == rows for r in y)
    assert [sk.decrypt(r) for r in y] == want
    xt = [[x[v][j] for v in range(n_vec)] for j in range(cols)]
    yt = pk.matmul(xt, wm, transposed=True)
    assert len(yt) == rows and all(len(r) == n_vec for r in yt)
    assert [sk.decrypt(r) for r in yt] == [[want[v][i] for v in range(n_vec)] for i in range(rows)]
    with pytest.raises(RuntimeError, match="matmul error: Size mismatch!"):
        pk.matmul(x, [[1, 2, 3]])
    with pytest.raises(RuntimeError, match="matmul error: negative weights have no encoding"):
        pk.matmul(x, [[1, 2, 3, 4, -5]])
