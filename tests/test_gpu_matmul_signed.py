"""The signed-weight encrypted matrix product on resident ciphertexts (pgpu_batch_ct_matmul_signed; matmul_signed_kernel of
csrc/hensel_signed.hpp, its host driver in csrc/capi_aggregate.inc) on the GPU:
    default      out[v*rows + i] = prod_j x[v*cols + j]^W[i][j] mod n^2
    transposed   out[i*n_vec + v] = prod_j x[j*n_vec + v]^W[i][j] mod n^2,     W[i][j] signed, two's complement in e_bits bits
held bit-identical to Python's pow with signed exponents, in both layouts, at the depth tests/test_gpu_matmul.py gives the
unsigned call: (5,13,33) under every forced window 1..6, slices (5 does not divide 33) and tiles (2: a short last pass;
transposed: staged, sliced and copied back); weight widths across the 64-bit word boundary with edge weights, stored bits
above e_bits and rows one word wider than e_bits needs; output counts around the 32 / 16 / 8 groups of a wavefront; key
widths off the standard classes and the refusal one bit beyond the last; inputs in every form a resident batch can have and
two layers chained through CRT decrypt; the refusal that follows the inversion, with the non-unit in the last tile; a call
whose short last pass runs on MORE slices than its full passes (plan.last_slices > plan.slices: 3072 and 2048 bits); and
ciphertext words uploaded with values at and above n^2.
The reference takes every inverse once: pow(x, e, n^2) with e < 0 is pow(pow(x, -1, n^2), -e, n^2), the same residue."""
import ctypes
import random

import pytest

from test_gpu_matmul import transpose
from test_gpu_matvec_signed import (INVALID, KIND_INVERT, KIND_MATMUL, NOT_INVERTIBLE, TRANSPOSED, UNSUPPORTED, Case, Ref,  # noqa: F401
                                    edge_matrix, knobs, signed_matrix)

pytestmark = pytest.mark.gpu
BITS = [1024, 2048, 3072]


class CachedRef(Ref):
    """Ref with pow(x, -1, n^2) taken once per x, and pow(x, e, n^2) once per (x, e) for |e| < 4 (the 2-bit weights)"""

    def __init__(self, nsq):
        super().__init__(nsq)
        self.inv, self.small = {}, {}

    def power(self, x, e):
        if e < 0:
            if x not in self.inv:
                self.inv[x] = pow(x, -1, self.nsq)
            x, e = self.inv[x], -e
        if e >= 4:
            return pow(x, e, self.nsq)
        if (x, e) not in self.small:
            self.small[(x, e)] = pow(x, e, self.nsq)
        return self.small[(x, e)]

    def row(self, xs, ws):
        acc = 1
        for x, e in zip(xs, ws):
            if e:
                acc = acc * self.power(x, e) % self.nsq
        return acc

    def matmul(self, xs, wm, n_vec):
        """default layout [n_vec][rows], from the flat [n_vec][cols] values"""
        cols = len(xs) // n_vec
        return [y for v in range(n_vec) for y in self.matvec(xs[v * cols:(v + 1) * cols], wm)]


def fetch(c, h):
    """download and free"""
    got = c.R.down(h)
    c.L.pgpu_batch_destroy(h)
    c.R.live.remove(h)
    return got


def plan_of(L, bits, n_vec, rows, cols, e_bits):
    pw, ps, pt = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    assert L.pgpu_ct_matmul_signed_plan(bits, n_vec, rows, cols, e_bits, ctypes.byref(pw), ctypes.byref(ps), ctypes.byref(pt), None, None) == 0
    return pw.value, ps.value, pt.value


def both_layouts(c, x, xt, w, n_vec, rows, e_bits, want, tag):
    """the default call on x, the transposed call on the same matrix of ciphertexts stored [cols][n_vec]"""
    assert fetch(c, c.matmul(x, w, n_vec, rows, e_bits)) == want, tag
    assert fetch(c, c.matmul(xt, w, n_vec, rows, e_bits, TRANSPOSED)) == transpose(want, n_vec, rows), (tag, "transposed")


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("e_bits", [13, 32])
def test_forced_windows_slices_and_tiles(engine, knobs, bits, e_bits):
    """(5,13,33), every window 1..6 (13 is no multiple of 2, 4, 5 or 6; 32 none of 3, 5 or 6: a top window narrower than w)
    x slices 1, 2, 5, 33 x tiles 1, 2, 5 in the default layout; the transposed layout staged, sliced and copied back
    (w4 S5 t2), staged and stored through the strides (w6 S1 t2), not staged and folded straight into the result (w3 S33
    t5), and (w1 S2 t1)"""
    c = Case(engine, bits)
    rng = random.Random(bits + e_bits)
    ref = CachedRef(c.nsq)
    n_vec, rows, cols = 5, 13, 33
    try:
        xs = c.units(rng, n_vec * cols)
        wm = signed_matrix(rng, rows, cols, e_bits)
        want = ref.matmul(xs, wm, n_vec)
        want_t = transpose(want, n_vec, rows)
        x, xt, w = c.up(xs), c.up(transpose(xs, n_vec, cols)), c.weights(wm, e_bits)
        for window in range(1, 7):
            for s in (1, 2, 5, 33):                       # 5 does not divide 33
                for t in (1, 2, 5):                       # 2: passes of 2, 2 and 1 vectors
                    knobs(matmul_window=window, matmul_slices=s, matmul_tile=t)
                    assert plan_of(c.L, bits, n_vec, rows, cols, e_bits) == (window, s, t)
                    assert fetch(c, c.matmul(x, w, n_vec, rows, e_bits)) == want, (window, s, t)
        for window, s, t in ((4, 5, 2), (6, 1, 2), (3, 33, 5), (1, 2, 1)):
            knobs(matmul_window=window, matmul_slices=s, matmul_tile=t)
            assert plan_of(c.L, bits, n_vec, rows, cols, e_bits) == (window, s, t)
            assert fetch(c, c.matmul(xt, w, n_vec, rows, e_bits, TRANSPOSED)) == want_t, (window, s, t)
        assert c.R.down(x) == xs                          # the operand is left as it was
    finally:
        c.R.close()


def wider_weights(c, wm, e_bits, rng):
    """rows one word wider than ceil(e_bits / 64), the extra word random: the cut of a window that runs off the last word
    e_bits needs reads it (word + 1 < w_words), the sign extension has to drop it again"""
    ew = (e_bits + 63) // 64
    flat = [(v & ((1 << e_bits) - 1)) | (rng.getrandbits(64) << (64 * ew)) for row in wm for v in row]
    return c.R.up(flat, ew + 1)


@pytest.mark.parametrize("e_bits", [1, 2, 8, 33, 64, 65, 70, 127])
def test_widths_edge_weights_and_ignored_bits(engine, knobs, e_bits):
    """every weight width; at 65, 70 and 127 every forced window: the look-behind bit of the window that starts at bit 64
    is bit 63 (w = 1, 2, 4), and for w = 3, 5, 6 a cut that starts at bits 59 .. 62 runs into the next word.  Rows of edge
    weights; each matrix uploaded clean, with random bits above e_bits inside its words, and in rows one word wider with
    the extra word random -- the same rows from all three, from the matvec call too"""
    c = Case(engine, 2048)
    rng = random.Random(e_bits + 40)
    ref = CachedRef(c.nsq)
    n_vec, cols = 3, 5
    try:
        xs = c.units(rng, n_vec * cols)
        wm = edge_matrix(rng, cols, e_bits)
        rows = len(wm)
        want = ref.matmul(xs, wm, n_vec)
        assert [want[v * rows] for v in range(n_vec)] == [1] * n_vec          # all-zero weights: the ciphertext 1
        x, xt, x0 = c.up(xs), c.up(transpose(xs, n_vec, cols)), c.up(xs[:cols])
        uploads = (c.weights(wm, e_bits), c.weights(wm, e_bits, garbage=rng), wider_weights(c, wm, e_bits, rng))
        for window in [None] + (list(range(1, 7)) if e_bits > 64 else []):
            knobs(**({} if window is None else {"matmul_window": window, "matvec_window": window}))
            for k, w in enumerate(uploads):
                both_layouts(c, x, xt, w, n_vec, rows, e_bits, want, (window, k))
            assert fetch(c, c.matvec(x0, uploads[2], rows, e_bits)) == want[:rows], window      # the wider rows, matvec
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", BITS)
def test_output_counts_around_a_wavefront(engine, knobs, bits):
    """one wavefront holds 32 / 16 / 8 outputs: 33, 16 and 8 outputs, one row, one vector, one column (forced slices clamp
    to 1) and nine; (7,5) under a tile of 2: the clamped dead groups of the last wavefront stay inside the tile"""
    c = Case(engine, bits)
    rng = random.Random(bits + 50)
    ref = CachedRef(c.nsq)
    try:
        pool = c.units(rng, 33 * 9)
        for n_vec, rows in ((1, 33), (3, 11), (2, 8), (2, 4), (7, 5), (33, 1)):
            for cols in (1, 9):
                xs = pool[:n_vec * cols]
                wm = signed_matrix(rng, rows, cols, 32)
                want = ref.matmul(xs, wm, n_vec)
                x, xt, w = c.up(xs), c.up(transpose(xs, n_vec, cols)), c.weights(wm, 32)
                plans = [{}] + ([{"matmul_slices": 3}] if cols == 1 else []) + ([{"matmul_tile": 2}] if (n_vec, rows) == (7, 5) else [])
                for plan in plans:
                    knobs(**plan)
                    _, s, t = plan_of(c.L, bits, n_vec, rows, cols, 32)
                    assert s <= cols and (cols > 1 or s == 1) and ("matmul_tile" not in plan or t == 2)
                    both_layouts(c, x, xt, w, n_vec, rows, 32, want, (n_vec, rows, cols, plan))
                c.R.close()
    finally:
        c.R.close()


def _edge_signed(rng, rows, cols):
    wm = signed_matrix(rng, rows, cols, 32)
    wm[0][:4] = [0, -1, -(1 << 31), (1 << 31) - 1]
    wm[1] = [0] * cols
    wm[2] = [-1] * cols
    return wm


@pytest.mark.parametrize("bits", [1065, 1124, 2051, 3211])
def test_key_widths_off_the_classes(engine, knobs, bits):
    """the last width of every pair-row class and 1124: 3 vectors of 7 under a signed 5 x 7 matrix, x in pair rows, both
    layouts, the plan's knobs and tiles of 2 over 3 slices; equal to pow, CRT-decrypting to W m mod n; the signed matvec on
    the first vector gives its rows"""
    from test_gpu_key_widths import Key
    K = Key(engine, bits)
    L, R = K.L, K.R
    rng = random.Random(bits + 60)
    ref = CachedRef(K.nsq)
    n_vec, rows, cols = 3, 5, 7
    try:
        x, m = K.fresh(rng, n_vec * cols)
        xs = R.down(x)
        xt = R.op(L.pgpu_batch_ct_add, K.pk._h, R.up(transpose(xs, n_vec, cols), 2 * K.nw), R.up([1], 2 * K.nw))    # pair rows too
        assert L.pgpu_batch_row_limbs(xt) == 2 * K.l2
        wm = _edge_signed(rng, rows, cols)
        w = R.up([v & 0xFFFFFFFF for row in wm for v in row], 1)
        want = ref.matmul(xs, wm, n_vec)
        plain = [sum(a * b for a, b in zip(row, m[v * cols:(v + 1) * cols])) % K.n for v in range(n_vec) for row in wm]
        for forced in ({}, {"matmul_tile": 2, "matmul_slices": 3}):
            knobs(**forced)
            if forced:
                assert plan_of(L, bits, n_vec, rows, cols, 32)[1:] == (3, 2)
            y = R.op(L.pgpu_batch_ct_matmul_signed, K.pk._h, x, w, n_vec, rows, 32, 0)
            assert L.pgpu_batch_count(y) == n_vec * rows and L.pgpu_batch_row_limbs(y) == 2 * K.l2
            assert R.down(y) == want, forced
            assert K.decrypt(y) == plain, forced
            yt = R.op(L.pgpu_batch_ct_matmul_signed, K.pk._h, xt, w, n_vec, rows, 32, TRANSPOSED)
            assert R.down(yt) == transpose(want, n_vec, rows), forced
            assert K.decrypt(yt) == transpose(plain, n_vec, rows), forced
        knobs()
        mv = R.op(L.pgpu_batch_ct_matvec_signed, K.pk._h, R.up(xs[:cols], 2 * K.nw), w, rows, 32)
        assert R.down(mv) == want[:rows]
        assert R.down(x) == xs
    finally:
        K.close()


def test_one_bit_beyond_the_last_class_is_refused(engine, knobs):
    """3212 bits: both signed calls and both signed plan queries return PGPU_ERR_UNSUPPORTED, *out stays null, nothing is
    launched"""
    from test_gpu_key_widths import Key
    K = Key(engine, 3212)
    L, R = K.L, K.R
    rng = random.Random(3212)
    try:
        x = R.up([rng.randrange(1, K.nsq) for _ in range(6)], 2 * K.nw)
        w = R.up([1, 2, 3, 4, 5, 6], 1)
        out = ctypes.c_void_p()
        kinds, forms, ms = (ctypes.c_int * 64)(), (ctypes.c_int * 64)(), (ctypes.c_double * 64)()
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            L.pgpu_timing_collect_ex(kinds, forms, ms, 64)
            assert L.pgpu_batch_ct_matvec_signed(K.pk._h, x, w, 1, 32, ctypes.byref(out)) == UNSUPPORTED
            assert b"pair" in L.pgpu_last_error() and not out.value
            for flags in (0, TRANSPOSED):                                        # 2 vectors of 3 under a 2 x 3 matrix
                assert L.pgpu_batch_ct_matmul_signed(K.pk._h, x, w, 2, 2, 32, flags, ctypes.byref(out)) == UNSUPPORTED
                assert b"pair" in L.pgpu_last_error() and not out.value
            assert L.pgpu_synchronize() == 0
            assert L.pgpu_timing_collect_ex(kinds, forms, ms, 64) == 0 and not out.value
        finally:
            L.pgpu_set_timing(0)
        a, b, t, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert L.pgpu_ct_matvec_signed_plan(3212, 1, 6, 32, ctypes.byref(a), ctypes.byref(b), ctypes.byref(tb), ctypes.byref(pr)) == UNSUPPORTED
        assert L.pgpu_ct_matmul_signed_plan(3212, 2, 2, 3, 32, ctypes.byref(a), ctypes.byref(b), ctypes.byref(t), ctypes.byref(tb),
                                            ctypes.byref(pr)) == UNSUPPORTED
        assert b"pair" in L.pgpu_last_error()
    finally:
        K.close()


@pytest.mark.parametrize("bits", BITS)
def test_input_forms_and_two_layers(engine, knobs, bits):
    """x as pair rows of a resident DJN encrypt, as pair rows out of pgpu_batch_ct_add, as Montgomery-form words (an encrypt
    with plaintext rows 2 nw words wide), as plain uploaded words: identical rows, x unchanged; then a second signed matmul
    on the first one's result, in both layouts, decrypting to W2 (W1 m) mod n with negative entries in both matrices"""
    c = Case(engine, bits)
    rng = random.Random(bits + 70)
    ref = CachedRef(c.nsq)
    L, R = c.L, c.R
    n_vec, cols, r1, r2, e_bits = 4, 11, 6, 3, 20
    try:
        m = [rng.randrange(c.n) for _ in range(n_vec * cols)]
        rw = bits // 128
        r = [rng.getrandbits(64 * rw) for _ in m]
        xa = R.op(L.pgpu_batch_encrypt, c.pk._h, R.up(m, c.nw), R.up(r, rw), 64 * rw)                  # (a) pair rows
        xs = R.down(xa)
        xb = R.op(L.pgpu_batch_ct_add, c.pk._h, c.up(xs), c.up([1]))                                  # (b) pair rows of CT + CT
        xc = R.op(L.pgpu_batch_encrypt, c.pk._h, R.up(m, 2 * c.nw), R.up(r, rw), 64 * rw)              # (c) Montgomery-form words
        xd = c.up(xs)                                                                                 # (d) plain words
        assert L.pgpu_batch_row_limbs(xa) > 0 and L.pgpu_batch_row_limbs(xb) > 0
        assert L.pgpu_batch_is_montgomery(xc) == 1 and L.pgpu_batch_row_limbs(xc) == 0
        assert L.pgpu_batch_is_montgomery(xd) == 0 and L.pgpu_batch_row_limbs(xd) == 0
        w1, w2 = signed_matrix(rng, r1, cols, e_bits), signed_matrix(rng, r2, r1, e_bits)
        assert all(any(v < 0 for row in wm for v in row) for wm in (w1, w2))
        wb1, wb2 = c.weights(w1, e_bits), c.weights(w2, e_bits)
        want = ref.matmul(xs, w1, n_vec)
        y = c.matmul(xa, wb1, n_vec, r1, e_bits)
        assert R.down(y) == want
        for k, xo in enumerate((xb, xc, xd)):
            assert R.down(c.matmul(xo, wb1, n_vec, r1, e_bits)) == want, k
        for xo in (xa, xb, xc, xd):
            assert R.down(xo) == xs                                  # x is left unchanged
        z = c.matmul(y, wb2, n_vec, r2, e_bits)                      # (e) a second layer on the first one's result
        assert R.down(z) == ref.matmul(want, w2, n_vec)
        d = c.decrypt(z)
        for v in range(n_vec):
            h = [sum(a * b for a, b in zip(row, m[v * cols:(v + 1) * cols])) for row in w1]
            assert d[v * r2:(v + 1) * r2] == [sum(a * b for a, b in zip(row, h)) % c.n for row in w2]
        # the transposed layers: Y = W1 X, Z = W2 Y on [cols][n_vec] storage
        yt = c.matmul(c.up(transpose(xs, n_vec, cols)), wb1, n_vec, r1, e_bits, TRANSPOSED)
        zt = c.matmul(yt, wb2, n_vec, r2, e_bits, TRANSPOSED)
        assert R.down(yt) == transpose(want, n_vec, r1)
        assert R.down(zt) == transpose(R.down(z), n_vec, r2)
    finally:
        R.close()


def test_a_non_unit_in_the_last_tile_is_refused_after_the_inversion(engine, knobs):
    """tile 2 over 5 vectors: the non-unit belongs to the last pass.  The inversion runs over all of x before the first
    pass: PGPU_ERR_NOT_INVERTIBLE, *out null, no launch of kind PGPU_KERNEL_MATMUL recorded; the next call is exact"""
    c = Case(engine, 2048)
    rng = random.Random(80)
    ref = CachedRef(c.nsq)
    L, R = c.L, c.R
    n_vec, rows, cols = 5, 3, 4
    try:
        xs = c.units(rng, n_vec * cols)
        wm = signed_matrix(rng, rows, cols, 32)
        w = c.weights(wm, 32)
        want = ref.matmul(xs, wm, n_vec)
        x, xt = c.up(xs), c.up(transpose(xs, n_vec, cols))
        out = ctypes.c_void_p()
        kinds, forms, ms = (ctypes.c_int * 256)(), (ctypes.c_int * 256)(), (ctypes.c_double * 256)()
        knobs(matmul_tile=2)
        assert plan_of(L, 2048, n_vec, rows, cols, 32)[2] == 2
        assert L.pgpu_synchronize() == 0
        assert L.pgpu_set_timing(1) == 0
        try:
            for bad in (c.p, c.n, 0):
                bad_xs = list(xs)
                bad_xs[4 * cols + 1] = bad                                        # vector 4: the last pass
                for flags, vals in ((0, bad_xs), (TRANSPOSED, transpose(bad_xs, n_vec, cols))):
                    assert vals[1 * n_vec + 4 if flags else 4 * cols + 1] == bad
                    xb = c.up(vals)
                    L.pgpu_timing_collect_ex(kinds, forms, ms, 256)               # drop what earlier calls left
                    assert L.pgpu_batch_ct_matmul_signed(c.pk._h, xb, w, n_vec, rows, 32, flags, ctypes.byref(out)) == NOT_INVERTIBLE
                    assert not out.value and b"unit" in L.pgpu_last_error()
                    assert L.pgpu_synchronize() == 0
                    n = L.pgpu_timing_collect_ex(kinds, forms, ms, 256)
                    seen = [kinds[i] for i in range(n)]
                    assert KIND_INVERT in seen and KIND_MATMUL not in seen, (bad == c.p, flags, seen)
                    both_layouts(c, x, xt, w, n_vec, rows, 32, want, ("after the refusal", flags))
        finally:
            L.pgpu_set_timing(0)
    finally:
        R.close()


@pytest.mark.parametrize("bits,n_vec,tile,rows,cols,s_full,s_last", [(3072, 9, 8, 512, 16, 2, 4), (2048, 9, 8, 512, 32, 4, 8),
                                                                     (3072, 5, 3, 560, 32, 5, 8)])
def test_last_pass_on_more_slices_than_a_full_pass(engine, knobs, bits, n_vec, tile, rows, cols, s_full, s_last):
    """no forced slices.  9 vectors in tiles of 8 at 3072 bits: a full pass has 4096 outputs = 512 wavefronts, fill 2 under
    the cap 16 / 4; the last pass of one vector 64 wavefronts, fill 16: four slices.  At 2048 bits: 256 and 32 wavefronts,
    four and eight slices of 32 columns; the fold picks its (4,18) / (8,9) form at two counts within one call.  5 vectors in
    tiles of 3, 70 wavefronts per vector: five slices of three vectors, then eight of two -- the short pass fills MORE of
    the partial block than a full one, which is why the block is sized by the larger count; the stage block is sized for a
    full tile.  Weights of 2 bits: {-2 .. 1}"""
    c = Case(engine, bits)
    rng = random.Random(bits + 90)
    ref = CachedRef(c.nsq)
    e_bits, last = 2, n_vec % tile
    try:
        knobs(matmul_tile=tile)
        full, one, whole = (plan_of(c.L, bits, k, rows, cols, e_bits) for k in (tile, last, n_vec))
        print(f"signed matmul plan, {bits} bits, tile {tile}: slices {full[1]} at n_vec = {tile}, {one[1]} at n_vec = {last}, {whole[1]} at n_vec = {n_vec}")
        assert (full[1], one[1]) == (s_full, s_last) and full[2] == tile
        assert whole[1:] == (s_full, tile) and one[0] == full[0] == whole[0]
        xs = c.units(rng, n_vec * cols)
        wm = signed_matrix(rng, rows, cols, e_bits)
        want = ref.matmul(xs, wm, n_vec)
        both_layouts(c, c.up(xs), c.up(transpose(xs, n_vec, cols)), c.weights(wm, e_bits), n_vec, rows, e_bits, want, (bits,))
    finally:
        c.R.close()


@pytest.mark.parametrize("bits", [2048, 2051])
def test_uploaded_words_at_and_above_n_squared(engine, knobs, bits):
    """an uploaded ciphertext batch has 2 nw words and may hold values in [n^2, 2^(128 nw)): n^2, n^2 + 1, 2^(128 nw) - 1
    and random full-width values.  CT + CT, CT x PT, negate, the signed matvec and CRT decrypt give, bit for bit, what they
    give on the values reduced modulo n^2; n^2 itself is 0: negate and the signed calls refuse it"""
    c = Case(engine, bits)
    rng = random.Random(bits + 100)
    ref = CachedRef(c.nsq)
    L, R = c.L, c.R
    try:
        full = 1 << (128 * c.nw)
        big = [c.nsq + 1, full - 1, rng.randrange(c.nsq, full) | (full >> 1), rng.randrange(c.nsq, full) | (full >> 1)]
        big = [v if (v % c.nsq) % c.p and (v % c.nsq) % c.q else v - 1 for v in big]
        assert all(c.nsq <= v < full and (v % c.nsq) % c.p and (v % c.nsq) % c.q for v in big)
        red = [v % c.nsq for v in big]
        other = c.units(rng, len(big))
        xb, xr, xo = c.up(big), c.up(red), c.up(other)
        e = [0, 1, (1 << 40) - 1, rng.getrandbits(40)]
        eb = R.up(e, 1)

        def same(fn, *tail):
            got, exp = R.down(R.op(fn, c.pk._h, xb, *tail)), R.down(R.op(fn, c.pk._h, xr, *tail))
            assert got == exp, fn
            return got
        assert same(L.pgpu_batch_ct_add, xo) == [a * b % c.nsq for a, b in zip(red, other)]
        assert R.down(R.op(L.pgpu_batch_ct_add, c.pk._h, xo, xb)) == [a * b % c.nsq for a, b in zip(red, other)]
        assert R.down(R.op(L.pgpu_batch_ct_add, c.pk._h, xb, xb)) == [a * a % c.nsq for a in red]
        assert same(L.pgpu_batch_ct_mul, eb, 40) == [pow(a, b, c.nsq) for a, b in zip(red, e)]
        assert same(L.pgpu_batch_ct_negate) == [pow(a, -1, c.nsq) for a in red]
        wm = signed_matrix(rng, 3, len(big), 32)
        assert same(L.pgpu_batch_ct_matvec_signed, c.weights(wm, 32), 3, 32) == ref.matvec(red, wm)
        assert c.decrypt(xb) == c.decrypt(xr)
        # n^2 itself, and n^2 among units: congruent to 0, no ciphertext
        out = ctypes.c_void_p()
        for vals in ([c.nsq], [big[0], c.nsq, big[1], big[2]]):
            z = c.up(vals)
            w = c.weights(wm[:1] if len(vals) == 4 else [[-3]], 32)
            assert L.pgpu_batch_ct_negate(c.pk._h, z, ctypes.byref(out)) == NOT_INVERTIBLE and not out.value
            assert L.pgpu_batch_ct_matvec_signed(c.pk._h, z, w, 1, 32, ctypes.byref(out)) == NOT_INVERTIBLE and not out.value
            assert L.pgpu_batch_ct_matmul_signed(c.pk._h, z, w, 1, 1, 32, 0, ctypes.byref(out)) == NOT_INVERTIBLE and not out.value
            assert R.down(R.op(L.pgpu_batch_ct_add, c.pk._h, z, z)) == [v * v % c.nsq for v in vals]      # (it still multiplies: 0)
            assert R.down(R.op(L.pgpu_batch_ct_mul, c.pk._h, z, R.up([5], 1), 40)) == [pow(v, 5, c.nsq) for v in vals]
        assert same(L.pgpu_batch_ct_negate) == [pow(a, -1, c.nsq) for a in red]                           # the lane stays usable
    finally:
        R.close()
