"""Signed-weight encrypted matvec and matmul on resident ciphertexts (pgpu_batch_ct_matvec_signed /
pgpu_batch_ct_matmul_signed; csrc/hensel_signed.hpp) on the GPU:
    out[i] = prod_j x[j]^W[i][j] mod n^2,   W[i][j] signed, two's complement in e_bits bits
held bit-identical to Python's pow with signed exponents (pow(x, -1, n^2) for the negative ones) for the 1024-, 2048- and
3072-bit key classes and one odd width (2051): shapes whose rows straddle a wavefront's groups and whose slices do not
divide the columns, forced windows 1..6 and slices, weight widths across the 64-bit word boundary, edge weights, stored
bits above e_bits, inputs in every form a resident batch can have, the agreement with sub(matvec(W+), matvec(W-)) and with
the unsigned call, the round trip through CRT decrypt, the matmul in both layouts with a staged and a shorter last pass
(its own depth: tests/test_gpu_matmul_signed.py), two lanes at once, the refusals -- the one that follows launches among them --, the timing record and the Python keyword."""
import ctypes
import json
import os
import random
import threading

import pytest

from test_gpu_pair_rows import Res, key_case

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden")
KIND_MATVEC, KIND_MATMUL, KIND_INVERT = 5, 11, 14    # include/pgpu.h: pgpu_kernel_kind
NOT_INVERTIBLE, UNSUPPORTED, INVALID = -6, -3, -1
TRANSPOSED = 1                                       # PGPU_MATMUL_TRANSPOSED
SHAPES = [(1, 1), (1, 7), (3, 1), (5, 33), (17, 9), (33, 5)]
KNOBS = ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES",
         "PGPU_INVERT_CHUNK", "PGPU_INVERT_WIDE")


class Case:
    def __init__(self, engine, bits):
        self.bits = bits
        if bits == 2051:
            k = [c for c in json.load(open(os.path.join(GOLD, "key_widths.json")))["cases"] if c["bits"] == bits][0]
            self.p, self.q, self.hs = int(k["p"], 16), int(k["q"], 16), None
        else:
            self.p, self.q, self.hs = key_case(bits, True)
        self.n = self.p * self.q
        assert self.n.bit_length() == bits
        self.nsq = self.n * self.n
        self.nw = (bits + 63) // 64
        self.pk, self.sk = engine.PublicKey(self.n, bits, hs=self.hs), engine.PrivateKey(self.p, self.q)
        self.R = Res()
        self.L = self.R.L

    def units(self, rng, count):
        out = []
        while len(out) < count:
            v = rng.randrange(1, self.nsq)
            if v % self.p and v % self.q:
                out.append(v)
        return out

    def up(self, xs):
        return self.R.up(xs, 2 * self.nw)

    def encrypt(self, m, rng):
        rw = self.bits // 128
        r = [rng.getrandbits(64 * rw) for _ in m]
        return self.R.op(self.L.pgpu_batch_encrypt, self.pk._h, self.R.up(m, self.nw), self.R.up(r, rw), 64 * rw)

    def weights(self, wm, e_bits, garbage=None):
        """the matrix as a plain uploaded batch: two's complement in ceil(e_bits / 64) words, optional bits above e_bits"""
        ew = (e_bits + 63) // 64
        flat = [v & ((1 << e_bits) - 1) for row in wm for v in row]
        if garbage is not None:
            flat = [(v | (garbage.getrandbits(64 * ew) << e_bits)) & ((1 << (64 * ew)) - 1) for v in flat]
        return self.R.up(flat, ew)

    def matvec(self, x, w, rows, e_bits):
        return self.R.op(self.L.pgpu_batch_ct_matvec_signed, self.pk._h, x, w, rows, e_bits)

    def matmul(self, x, w, n_vec, rows, e_bits, flags=0):
        return self.R.op(self.L.pgpu_batch_ct_matmul_signed, self.pk._h, x, w, n_vec, rows, e_bits, flags)

    def decrypt(self, h):
        return self.R.down(self.R.op(self.L.pgpu_batch_decrypt_crt, self.sk._h, h))


class Ref:
    """pow(x, d, n^2) for the digits one vector meets, shared by the tests of a key: x and x^-1 once, small exponents after"""

    def __init__(self, nsq):
        self.nsq = nsq

    def row(self, xs, ws):
        acc = 1
        for x, e in zip(xs, ws):
            acc = acc * pow(x, e, self.nsq) % self.nsq
        return acc

    def matvec(self, xs, wm):
        return [self.row(xs, row) for row in wm]


def signed_matrix(rng, rows, cols, e_bits):
    top = 1 << (e_bits - 1)
    return [[rng.randrange(-top, top) for _ in range(cols)] for _ in range(rows)]


def edge_matrix(rng, cols, e_bits):
    """rows: all 0, all -1, all -2^(e-1), all 2^(e-1)-1, alternating signs, random"""
    top = 1 << (e_bits - 1)
    alt = [(top - 1 if j % 2 else -top) if e_bits > 1 else -(j % 2) for j in range(cols)]
    return [[0] * cols, [-1] * cols, [-top] * cols, [top - 1] * cols, alt, [rng.randrange(-top, top) for _ in range(cols)]]


@pytest.fixture
def knobs(monkeypatch):
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)

    def force(**kw):
        for name in KNOBS:
            monkeypatch.delenv(name, raising=False)
        for name, v in kw.items():
            monkeypatch.setenv("PGPU_" + name.upper(), str(v))
    return force


@pytest.mark.parametrize("bits", [1024, 2048, 3072, 2051])
def test_exact_at_every_shape(engine, knobs, bits):
    """uploaded words; rows 1 .. 33 straddle the 32 / 16 / 8 groups of a wavefront, 33 and 9 columns are cut into slices
    that do not divide them"""
    c = Case(engine, bits)
    rng = random.Random(bits)
    ref = Ref(c.nsq)
    try:
        pool = c.units(rng, 33)
        for rows, cols in SHAPES:
            xs = pool[:cols]
            wm = signed_matrix(rng, rows, cols, 32)
            y = c.matvec(c.up(xs), c.weights(wm, 32), rows, 32)
            assert c.L.pgpu_batch_count(y) == rows and c.L.pgpu_batch_row_limbs(y) > 0
            assert c.R.down(y) == ref.matvec(xs, wm), (rows, cols)
            c.R.close()
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_forced_windows_and_slices(engine, knobs, bits):
    c = Case(engine, bits)
    rng = random.Random(bits + 1)
    ref = Ref(c.nsq)
    try:
        rows, cols = 5, 9
        xs = c.units(rng, cols)
        wm = signed_matrix(rng, rows, cols, 32)
        want = ref.matvec(xs, wm)
        x, w = c.up(xs), c.weights(wm, 32)
        pw, ps, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
        for window in range(1, 7):
            for slices in (1, 2, cols):
                knobs(matvec_window=window, matvec_slices=slices)
                assert c.L.pgpu_ct_matvec_signed_plan(bits, rows, cols, 32, ctypes.byref(pw), ctypes.byref(ps), ctypes.byref(tb),
                                                      ctypes.byref(pr)) == 0
                assert (pw.value, ps.value) == (window, slices)
                assert c.R.down(c.matvec(x, w, rows, 32)) == want, (window, slices)
    finally:
        c.R.close()


@pytest.mark.parametrize("e_bits", [1, 2, 8, 32, 33, 64, 65, 70])
def test_widths_edge_weights_and_ignored_bits(engine, knobs, e_bits):
    """every weight width, 64 and 65 / 70 across the word boundary; at 65 and 70 forced windows 1, 2 and 4 start a window
    exactly at bit 64, so that its look-behind bit lies in the word before.  Rows of edge weights; stored bits above e_bits
    are random and must be ignored"""
    c = Case(engine, 2048)
    rng = random.Random(e_bits)
    ref = Ref(c.nsq)
    try:
        cols = 5
        xs = c.units(rng, cols)
        wm = edge_matrix(rng, cols, e_bits)
        want = ref.matvec(xs, wm)
        assert want[0] == 1                                  # all-zero weights: the ciphertext 1
        x = c.up(xs)
        w_clean, w_dirty = c.weights(wm, e_bits), c.weights(wm, e_bits, garbage=rng)
        for window in [None] + ([1, 2, 4] if e_bits > 64 else []):
            knobs(**({} if window is None else {"matvec_window": window}))
            assert c.R.down(c.matvec(x, w_clean, len(wm), e_bits)) == want, window
            assert c.R.down(c.matvec(x, w_dirty, len(wm), e_bits)) == want, window
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", [1024, 2048, 3072])
def test_input_forms_other_routes_and_decrypt(engine, knobs, bits):
    """x as pair rows from a resident encrypt and as uploaded words, with the ciphertexts 1 and n^2 - 1 among them; the
    result equals sub(matvec(x, W+), matvec(x, W-)) bit for bit, for non-negative weights the unsigned call at e_bits - 1,
    and decrypts to W * m mod n"""
    c = Case(engine, bits)
    rng = random.Random(bits + 2)
    ref = Ref(c.nsq)
    L = c.L
    try:
        rows, cols, e_bits = 4, 7, 20
        m = [rng.randrange(c.n) for _ in range(cols)]
        xe = c.encrypt(m, rng)                               # pair rows
        xs = c.R.down(xe)
        wm = signed_matrix(rng, rows, cols, e_bits)
        w = c.weights(wm, e_bits)
        y = c.matvec(xe, w, rows, e_bits)
        want = ref.matvec(xs, wm)
        assert c.R.down(y) == want
        assert c.R.down(c.matvec(c.up(xs), w, rows, e_bits)) == want         # uploaded words
        assert c.decrypt(y) == [sum(a * b for a, b in zip(row, m)) % c.n for row in wm]
        assert c.R.down(xe) == xs                                            # the operand is left as it was
        # the composed route of the parent: two unsigned matvecs and a subtraction
        wp = c.R.up([max(v, 0) for row in wm for v in row], 1)
        wn = c.R.up([max(-v, 0) for row in wm for v in row], 1)
        yp = c.R.op(L.pgpu_batch_ct_matvec, c.pk._h, xe, wp, rows, e_bits)
        yn = c.R.op(L.pgpu_batch_ct_matvec, c.pk._h, xe, wn, rows, e_bits)
        assert c.R.down(c.R.op(L.pgpu_batch_ct_sub, c.pk._h, yp, yn)) == want
        # non-negative weights: the unsigned call at e_bits - 1
        wu = [[abs(v) >> 1 for v in row] for row in wm]
        wub = c.R.up([v for row in wu for v in row], 1)
        assert c.R.down(c.matvec(xe, wub, rows, e_bits)) == c.R.down(c.R.op(L.pgpu_batch_ct_matvec, c.pk._h, xe, wub, rows, e_bits - 1))
        # the ciphertexts 1 and n^2 - 1 among the inputs
        xs2 = [1, c.nsq - 1] + xs[2:]
        assert c.R.down(c.matvec(c.up(xs2), w, rows, e_bits)) == ref.matvec(xs2, wm)
    finally:
        c.R.close()


@pytest.mark.parametrize("bits,n_vec", [(2048, 1), (2048, 3), (2048, 9), (1024, 3), (3072, 3)])
def test_matmul_both_layouts_and_staged_passes(engine, knobs, bits, n_vec):
    """default plan and a forced tile of 2 < n_vec: a staged transposed pass and a shorter last pass (n_vec odd); one and
    three slices"""
    c = Case(engine, bits)
    rng = random.Random(bits + n_vec)
    ref = Ref(c.nsq)
    try:
        rows, cols, e_bits = 5, 7, 32
        xs = c.units(rng, n_vec * cols)
        wm = signed_matrix(rng, rows, cols, e_bits)
        w = c.weights(wm, e_bits)
        want = [ref.matvec(xs[v * cols:(v + 1) * cols], wm) for v in range(n_vec)]           # [n_vec][rows]
        flat = [y for v in want for y in v]
        xt = [xs[v * cols + j] for j in range(cols) for v in range(n_vec)]                   # [cols][n_vec]
        flat_t = [want[v][i] for i in range(rows) for v in range(n_vec)]                     # [rows][n_vec]
        x, xtb = c.up(xs), c.up(xt)
        plans = [{}] + ([{"matmul_tile": 2, "matmul_slices": s} for s in (1, 3)] if n_vec > 2 else [])
        for plan in plans:
            knobs(**plan)
            if plan:
                pt = ctypes.c_size_t()
                assert c.L.pgpu_ct_matmul_signed_plan(bits, n_vec, rows, cols, e_bits, None, None, ctypes.byref(pt), None, None) == 0
                assert pt.value == 2
            assert c.R.down(c.matmul(x, w, n_vec, rows, e_bits)) == flat, plan
            assert c.R.down(c.matmul(xtb, w, n_vec, rows, e_bits, TRANSPOSED)) == flat_t, plan
        knobs()
        if n_vec == 1:
            assert c.R.down(c.matvec(x, w, rows, e_bits)) == flat
    finally:
        c.R.close()


def test_two_lanes_at_once(engine, knobs):
    """two threads on different batch lanes, each with its own x, the matrices uploaded by the main thread on its lane: a
    signed matvec 17 x 40 beside a signed matmul, transposed, tile 2 and 3 slices (staged, sliced, copied back), 5 vectors
    of 7 -> 5.  Each call blocks on the inversion's host round trip and takes up to four workspaces from its lane's arena;
    three calls in a row per thread; one run"""
    c = Case(engine, 2048)
    L = c.L
    rng = random.Random(12)
    ref = Ref(c.nsq)
    results, errors = {}, []
    shapes = {1: (1, 17, 40), 2: (5, 5, 7)}                # lane: n_vec, rows, cols
    wms = {lane: signed_matrix(rng, rows, cols, 32) for lane, (_, rows, cols) in shapes.items()}
    xss = {lane: c.units(rng, n_vec * cols) for lane, (n_vec, _, cols) in shapes.items()}      # lane 2: stored [cols][n_vec]
    knobs(matmul_tile=2, matmul_slices=3)

    def worker(lane):
        R = Res()
        try:
            R.check(L.pgpu_set_batch_lane(lane))
            n_vec, rows, cols = shapes[lane]
            x = R.up(xss[lane], 2 * c.nw)
            assert L.pgpu_batch_lane(x) == lane
            for it in range(3):
                if lane == 1:
                    y = R.op(L.pgpu_batch_ct_matvec_signed, c.pk._h, x, ws[lane], rows, 32)
                else:
                    y = R.op(L.pgpu_batch_ct_matmul_signed, c.pk._h, x, ws[lane], n_vec, rows, 32, TRANSPOSED)
                assert L.pgpu_batch_lane(y) == lane
                results[(lane, it)] = R.down(y)
        except Exception as ex:      # noqa: BLE001 -- reported by the main thread
            errors.append((lane, repr(ex)))
        finally:
            R.close()

    try:
        ws = {lane: c.weights(wms[lane], 32) for lane in shapes}     # lane of the main thread: ordered in by events
        pt = ctypes.c_size_t()
        assert L.pgpu_ct_matmul_signed_plan(2048, 5, 5, 7, 32, None, None, ctypes.byref(pt), None, None) == 0 and pt.value == 2
        ts = [threading.Thread(target=worker, args=(lane,)) for lane in (1, 2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        assert not errors, errors
        assert len(results) == 6
        want1 = ref.matvec(xss[1], wms[1])
        by_vec = [ref.matvec([xss[2][j * 5 + v] for j in range(7)], wms[2]) for v in range(5)]
        want2 = [by_vec[v][i] for i in range(5) for v in range(5)]                           # [rows][n_vec]
        for it in range(3):
            assert results[(1, it)] == want1, it
            assert results[(2, it)] == want2, it
    finally:
        c.R.close()


def test_refusals(engine, knobs):
    c = Case(engine, 2048)
    rng = random.Random(5)
    ref = Ref(c.nsq)
    L = c.L
    try:
        rows, cols = 3, 4
        xs = c.units(rng, cols)
        wm = signed_matrix(rng, rows, cols, 32)
        x, w = c.up(xs), c.weights(wm, 32)
        out = ctypes.c_void_p()

        def mv(*a):
            return L.pgpu_batch_ct_matvec_signed(*a, ctypes.byref(out))

        def mm(*a):
            return L.pgpu_batch_ct_matmul_signed(*a, ctypes.byref(out))
        # the one refusal that follows launches: an element that is no unit modulo n^2; the lane stays usable
        for bad in (c.n, 0, c.p):
            xb = c.up([xs[0], bad] + xs[2:])
            assert mv(c.pk._h, xb, w, rows, 32) == NOT_INVERTIBLE and not out.value
            assert mm(c.pk._h, xb, w, 1, rows, 32, 0) == NOT_INVERTIBLE and not out.value
            assert c.R.down(c.matvec(x, w, rows, 32)) == ref.matvec(xs, wm)
        # null arguments, sizes, e_bits, the matrix's form
        assert mv(None, x, w, rows, 32) == INVALID and mv(c.pk._h, None, w, rows, 32) == INVALID and mv(c.pk._h, x, None, rows, 32) == INVALID
        assert L.pgpu_batch_ct_matvec_signed(c.pk._h, x, w, rows, 32, None) == INVALID
        assert mv(c.pk._h, x, w, 0, 32) == INVALID
        assert mv(c.pk._h, x, w, rows + 1, 32) == INVALID and b"Size mismatch" in L.pgpu_last_error()
        assert mv(c.pk._h, x, w, rows, 0) == INVALID and b"e_bits" in L.pgpu_last_error()
        assert mv(c.pk._h, x, w, rows, 65) == INVALID and b"e_bits" in L.pgpu_last_error()
        assert mv(c.pk._h, w, w, rows, 32) == INVALID and b"width" in L.pgpu_last_error()
        assert mv(c.pk._h, x, c.encrypt([1] * (rows * cols), rng), rows, 32) == INVALID and b"plain uploaded" in L.pgpu_last_error()
        assert mm(c.pk._h, x, w, 0, rows, 32, 0) == INVALID and mm(c.pk._h, x, w, 3, rows, 32, 0) == INVALID
        assert mm(c.pk._h, x, w, 1, rows, 32, 2) == INVALID and b"flag" in L.pgpu_last_error()
        assert mm(c.pk._h, x, w, 1, rows, 0, 0) == INVALID and mm(c.pk._h, x, w, 1, rows, 65, 0) == INVALID
        assert mm(c.pk._h, x, w, 2, rows, 32, 0) == INVALID and b"Size mismatch" in L.pgpu_last_error()
        assert not out.value
        # the masked table-gather policy
        assert L.pgpu_set_table_gather_policy(1) == 0
        try:
            assert mv(c.pk._h, x, w, rows, 32) == UNSUPPORTED and b"masked" in L.pgpu_last_error() and not out.value
            assert mm(c.pk._h, x, w, 1, rows, 32, 0) == UNSUPPORTED and b"masked" in L.pgpu_last_error() and not out.value
        finally:
            L.pgpu_set_table_gather_policy(0)
        assert c.R.down(c.matvec(x, w, rows, 32)) == ref.matvec(xs, wm)
        # plan queries
        assert L.pgpu_ct_matvec_signed_plan(4096, 4, 4, 32, None, None, None, None) == UNSUPPORTED
        assert L.pgpu_ct_matmul_signed_plan(4096, 2, 4, 4, 32, None, None, None, None, None) == UNSUPPORTED
        assert L.pgpu_ct_matmul_signed_plan(2048, 0, 4, 4, 32, None, None, None, None, None) == INVALID
    finally:
        c.R.close()


def test_timing_record_kinds(engine, knobs):
    """the inversion's launches (PGPU_KERNEL_INVERT) come first, then the call's own: table build, multi-exponentiation and
    fold, all of kind PGPU_KERNEL_MATVEC / PGPU_KERNEL_MATMUL"""
    c = Case(engine, 2048)
    rng = random.Random(6)
    L = c.L
    try:
        rows, cols = 3, 8
        x = c.encrypt([rng.randrange(c.n) for _ in range(cols)], rng)
        w = c.weights(signed_matrix(rng, rows, cols, 32), 32)
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        knobs(matvec_slices=2, matmul_slices=2)
        assert L.pgpu_set_timing(1) == 0
        try:
            for call, kind in ((lambda: c.matvec(x, w, rows, 32), KIND_MATVEC), (lambda: c.matmul(x, w, 1, rows, 32), KIND_MATMUL)):
                L.pgpu_timing_collect_ex(kinds, forms, ms, 64)             # drop what earlier calls left
                call()
                assert L.pgpu_synchronize() == 0
                n = L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
                seen = [kinds[i] for i in range(n)]
                assert seen.count(KIND_INVERT) >= 2                        # forward passes and walks back of 8 elements
                last = max(i for i in range(n) if seen[i] == KIND_INVERT)  # (the grand total's conversions lie between them)
                assert kind not in seen[:last]
                assert seen[last + 1:] == [kind] * 3                       # table, multi-exponentiation, one fold level
        finally:
            L.pgpu_set_timing(0)
    finally:
        c.R.close()


def test_python_keyword(engine, knobs):
    p, q, hs = key_case(2048, True)
    n = p * q
    nsq = n * n
    pk, sk = engine.PublicKey(n, 2048, hs=hs), engine.PrivateKey(p, q)
    rng = random.Random(8)
    m = [rng.randrange(n) for _ in range(6)]
    ct = pk.encrypt(m, [rng.getrandbits(1024) for _ in m])
    wm = [[-3, 0, 7, -(1 << 40), 5, -1], [1, 2, 3, 4, 5, 6], [0] * 6]
    y = pk.matvec(ct, wm, signed=True)
    assert y == Ref(nsq).matvec(ct, wm)
    assert sk.decrypt(y) == [sum(a * b for a, b in zip(row, m)) % n for row in wm]
    assert pk.matvec(ct, wm[1]) == pk.matvec(ct, wm[1], signed=True)            # one flat row: a dot product
    xs = [ct[:3], ct[3:]]
    w2 = [[-1, 2, -3], [4, -5, 6]]
    out = pk.matmul(xs, w2, signed=True)
    assert out == [Ref(nsq).matvec(v, w2) for v in xs]
    out_t = pk.matmul([list(col) for col in zip(*xs)], w2, transposed=True, signed=True)
    assert out_t == [list(r) for r in zip(*out)]
    with pytest.raises(RuntimeError, match="negative weights have no encoding"):
        pk.matvec(ct, wm)
    with pytest.raises(RuntimeError, match="negative weights have no encoding"):
        pk.matmul(xs, w2)
