"""The signed-weight encrypted matvec / matmul (pgpu_batch_ct_matvec_signed / _matmul_signed; csrc/hensel_signed.hpp) on
the CPU, in plain Python ints.

1. The radix-2^w Booth recoding of a two's-complement weight of e_bits bits,
       d_k = -2^(w-1) b[kw+w-1] + sum_{i<w-1} 2^i b[kw+i] + b[kw-1],   b[-1] = 0,  b[i] = b[e_bits-1] for i >= e_bits,
   as the formula states it and as the kernel cuts it out of 64-bit words (signed_digit_row: one look-behind bit, across
   word boundaries, the top window sign-extended, stored bits at and above e_bits ignored): exhaustive for e_bits <= 10,
   edge values and random ones beyond.
2. The whole schedule: the batched inversion (forward running products, ONE inversion, the walk back), the table of
   2h + 1 rows per element over [x ; x^-1], the top-down walk per (row, column slice), the fold -- against
   prod_j pow(x_j, W_ij, n^2) with Python's signed exponents, and its executed products against the plan formula
   (csrc/policy.cpp: matvec_signed_products = the unsigned count + 3 (cols - 1)).
3. The passes of pgpu_batch_ct_matmul_signed with the ADDRESSES csrc/capi_aggregate.inc and matmul_signed_kernel form, on
   bounds-checked flat blocks for x, x^-1, stage, table, partial and out: x_off per layout, the two 2-D copies into
   [2][tile * cols], the table of 2^w + 1 rows per element and its two strides, the output strides for one slice and for
   several, the fold's walk and destination, the copy back with pitch n_vec, a short last pass on its own slice count --
   every output written exactly once with the pow value, no row outside a block touched, none read before it was written.
4. The contract of the host-side plan queries pgpu_ct_matvec_signed_plan / pgpu_ct_matmul_signed_plan (ctypes; no device)."""
import ctypes
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
E_BITS = [1, 2, 5, 31, 32, 33, 63, 64, 65, 70, 128]
WINDOWS = [1, 2, 3, 4, 5, 6]
CAP = 256 << 20                                   # policy.hpp: kMatvecTableCap
ROW_BYTES = {1024: 2 * 2 * 19 * 4, 2048: 2 * 4 * 18 * 4, 3072: 2 * 8 * 14 * 4}


def signed_value(stored, e_bits):
    """the weight a stored value stands for: its low e_bits bits as two's complement"""
    v = stored & ((1 << e_bits) - 1)
    return v - (1 << e_bits) if v >> (e_bits - 1) else v


def booth_formula(stored, e_bits, w):
    """the digits as the formula above states them, lowest window first"""
    nwin = (e_bits + w - 1) // w

    def b(i):
        if i < 0:
            return 0
        return (stored >> min(i, e_bits - 1)) & 1
    return [-(1 << (w - 1)) * b(k * w + w - 1) + sum(b(k * w + i) << i for i in range(w - 1)) + b(k * w - 1)
            for k in range(nwin)]


def kernel_row(stored, w_words, e_bits, w, win):
    """csrc/hensel_signed.hpp: signed_digit_row -- the table row window `win` selects, cut out of 64-bit words"""
    ep = [(stored >> (64 * k)) & M64 for k in range(w_words)]
    nwin = (e_bits + w - 1) // w
    top_bits = e_bits - (nwin - 1) * w + 1
    if win == 0:
        u = (ep[0] << 1) & M64
    else:
        bit = win * w - 1
        word, sh = bit >> 6, bit & 63
        assert word < w_words
        u = ep[word] >> sh
        if sh + w + 1 > 64 and word + 1 < w_words:
            u |= (ep[word + 1] << (64 - sh)) & M64
    if win == nwin - 1:
        assert 2 <= top_bits <= w + 1
        u &= (1 << top_bits) - 1
        if u >> (top_bits - 1):
            u |= M64 ^ ((1 << top_bits) - 1)
    h = 1 << (w - 1)
    c = u & (2 * h - 1)
    d = (c >> 1) + (c & 1) - ((u >> w) & 1) * h
    return d if d >= 0 else h - d


def row_of(d, w):
    h = 1 << (w - 1)
    return d if d >= 0 else h - d


def edge_values(e_bits):
    top = 1 << (e_bits - 1)
    alt = sum(1 << i for i in range(0, e_bits, 2))
    cand = {0, 1, -1, -top, top - 1, signed_value(alt, e_bits), signed_value(alt << 1, e_bits)}
    return sorted(v for v in cand if -top <= v < top)


def check_recoding(value, e_bits, w, garbage=0):
    w_words = (e_bits + 63) // 64
    stored = (value & ((1 << e_bits) - 1)) | (garbage << e_bits)
    stored &= (1 << (64 * w_words)) - 1
    ds = booth_formula(stored, e_bits, w)
    h = 1 << (w - 1)
    assert all(-h <= d <= h for d in ds)
    assert sum(d << (k * w) for k, d in enumerate(ds)) == value
    assert [kernel_row(stored, w_words, e_bits, w, k) for k in range(len(ds))] == [row_of(d, w) for d in ds]


@pytest.mark.parametrize("w", WINDOWS)
def test_recoding_exhaustive_small_widths(w):
    for e_bits in range(1, 11):
        for value in range(-(1 << (e_bits - 1)), 1 << (e_bits - 1)):
            check_recoding(value, e_bits, w)
            check_recoding(value, e_bits, w, garbage=(1 << 64) - 1)     # stored bits above e_bits are ignored
            check_recoding(value, e_bits, w, garbage=0x5A5A5A5A5A5A5A5)


@pytest.mark.parametrize("e_bits", E_BITS)
@pytest.mark.parametrize("w", WINDOWS)
def test_recoding_edges_and_word_boundaries(e_bits, w):
    rng = random.Random(100 * e_bits + w)
    top = 1 << (e_bits - 1)
    values = edge_values(e_bits) + [rng.randrange(-top, top) for _ in range(40)]
    for value in values:
        for garbage in (0, rng.getrandbits(64), (1 << 64) - 1):
            check_recoding(value, e_bits, w, garbage)


# ---- the schedule ----
def invert_batch(xs, mod):
    """simultaneous inversion as the batched inversion runs it (one chain here): -> (inverses, products)"""
    run, n = [xs[0] % mod], 0
    for x in xs[1:]:
        run.append(run[-1] * x % mod)
        n += 1
    u = pow(run[-1], -1, mod)                     # the ONE inversion (the host's)
    inv = [None] * len(xs)
    for i in range(len(xs) - 1, 0, -1):
        inv[i] = u * run[i - 1] % mod
        u = u * xs[i] % mod
        n += 2
    inv[0] = u
    return inv, n


def model(xs, wm, mod, e_bits, w, slices):
    """-> (results, executed products: inversion, table, squarings, multiplications, fold); wm: stored weights"""
    rows, cols = len(wm), len(xs)
    w_words = (e_bits + 63) // 64
    assert 1 <= slices <= cols
    nwin = (e_bits + w - 1) // w
    h = 1 << (w - 1)
    xinv, n_inv = invert_batch(xs, mod)
    n_table = n_sq = n_mul = n_fold = 0
    table = []
    for x, xi in zip(xs, xinv):                   # matvec_signed_table_kernel: one group per (element, half)
        t = [None] * (2 * h + 1)
        t[0] = 1 % mod
        for half, base in ((0, x % mod), (1, xi)):
            r0 = half * h
            t[r0 + 1] = base
            for e in range(2, h + 1):
                t[r0 + e] = t[r0 + e - 1] * base % mod
                n_table += 1
        assert None not in t
        table.append(t)
    part = [[None] * rows for _ in range(slices)]
    for s in range(slices):                       # matvec_signed_kernel: one group per (row, slice)
        lo, hi = s * cols // slices, (s + 1) * cols // slices
        assert lo < hi
        for i in range(rows):
            acc = table[lo][kernel_row(wm[i][lo], w_words, e_bits, w, nwin - 1)]    # the first position is a load
            for win in range(nwin - 1, -1, -1):
                if win != nwin - 1:
                    for _ in range(w):
                        acc = acc * acc % mod
                        n_sq += 1
                for j in range(lo + 1 if win == nwin - 1 else lo, hi):
                    acc = acc * table[j][kernel_row(wm[i][j], w_words, e_bits, w, win)] % mod   # (digit 0: times one)
                    n_mul += 1
            part[s][i] = acc
    cur = slices                                  # the unchanged fold
    while cur > 1:
        hh = (cur + 1) // 2
        for k in range(cur - hh):
            for i in range(rows):
                part[k][i] = part[k][i] * part[k + hh][i] % mod
                n_fold += 1
        cur = hh
    return part[0], (n_inv, n_table, n_sq, n_mul, n_fold)


def reference(xs, wm, mod, e_bits):
    out = []
    for row in wm:
        acc = 1 % mod
        for x, e in zip(xs, row):
            acc = acc * pow(x, signed_value(e, e_bits), mod) % mod
        out.append(acc)
    return out


def planned_products(rows, cols, e_bits, w, slices):
    """csrc/policy.cpp: matvec_signed_products"""
    return (cols * ((1 << w) - 2) + rows * slices * e_bits + rows * cols * ((e_bits + w - 1) // w) + rows * (slices - 1)
            + 3 * (cols - 1))


def stored_weights(rng, rows, cols, e_bits):
    mask, top = (1 << e_bits) - 1, 1 << (e_bits - 1)
    w_words = (e_bits + 63) // 64
    room = 64 * w_words - e_bits
    wm = [[rng.getrandbits(e_bits) | (rng.getrandbits(room) << e_bits if room else 0) for _ in range(cols)] for _ in range(rows)]
    fixed = [0, -1 & mask, top, top - 1, sum(1 << i for i in range(0, e_bits, 2))]      # 0, -1, -2^(e-1), 2^(e-1)-1, alternating
    for i, v in enumerate(fixed[:rows]):
        wm[i] = [v] * cols
    return wm


@pytest.mark.parametrize("e_bits", E_BITS)
@pytest.mark.parametrize("w", WINDOWS)
def test_schedule_model(e_bits, w):
    rng = random.Random(1000 * e_bits + w)
    for cols in (1, 2, 7):
        p, q = rng.choice([(1009, 1013), (65521, 65537)])
        n = p * q
        mod = n * n
        rows = 6
        xs = ([1, mod - 1] + [rng.randrange(1, mod) for _ in range(cols)])[:cols]
        xs = [x if x % p and x % q else x + 1 for x in xs]
        wm = stored_weights(rng, rows, cols, e_bits)
        want = reference(xs, wm, mod, e_bits)
        assert want[0] == 1
        for slices in sorted({1, 2, 3, cols}):
            if slices > cols:
                continue
            got, (ni, nt, ns, nm, nf) = model(xs, wm, mod, e_bits, w, slices)
            assert got == want, (cols, slices)
            nwin = (e_bits + w - 1) // w
            assert ni == 3 * (cols - 1)
            assert nt == cols * ((1 << w) - 2)                    # 2 (h - 1): as many as the unsigned table
            assert ns == rows * slices * (nwin - 1) * w          # the top window needs no squarings
            assert nm == rows * (cols * nwin - slices)           # the first position of every group is a load
            assert nf == rows * (slices - 1)
            assert ni + nt + ns + nm + nf <= planned_products(rows, cols, e_bits, w, slices)


def test_w4_e32_against_pow():
    rng = random.Random(7)
    mod = (251 * 241) ** 2
    xs = [rng.randrange(2, mod) for _ in range(5)]
    xs = [x if x % 251 and x % 241 else x + 1 for x in xs]
    wm = [[rng.getrandbits(32) for _ in xs] for _ in range(8)]
    assert any(signed_value(v, 32) < 0 for r in wm for v in r)
    assert model(xs, wm, mod, 32, 4, 2)[0] == reference(xs, wm, mod, 32)


# ---- the signed matmul's addressing ----
class Block:
    """a device block as a flat list of rows: every access is bounds-checked, and a row is read only after it was written"""

    def __init__(self, name, rows, fill=None):
        self.name, self.v = name, [None] * rows if fill is None else list(fill)
        assert len(self.v) == rows

    def rd(self, i):
        assert 0 <= i < len(self.v), (self.name, "read outside the block", i, len(self.v))
        assert self.v[i] is not None, (self.name, "read before written", i)
        return self.v[i]

    def wr(self, i, val, once=False):
        assert 0 <= i < len(self.v), (self.name, "write outside the block", i, len(self.v))
        assert not once or self.v[i] is None, (self.name, "written twice", i)
        self.v[i] = val

    def clear(self):
        self.v = [None] * len(self.v)

    def written(self):
        return [i for i, r in enumerate(self.v) if r is not None]


def copy2d(dst, d0, dpitch, src, s0, spitch, width, height, once=False):
    """hipMemcpy2DAsync in rows: height lines of width rows, the pitches in rows too"""
    for line in range(height):
        for k in range(width):
            dst.wr(d0 + line * dpitch + k, src.rd(s0 + line * spitch + k), once)


def matmul_signed_model(xs, wm, mod, n_vec, transposed, e_bits, w, tile, slices, last_slices, g, w_words=None):
    """the passes of pgpu_batch_ct_matmul_signed as capi_aggregate.inc sets them up, on flat blocks of rows: -> the result
    batch.  wm: stored weights; slices / last_slices: the plan's counts for a full pass and for the last one"""
    rows, cols = len(wm), len(xs) // n_vec
    w_words = w_words or (e_bits + 63) // 64
    ipw, nwin, h = 64 // g, (e_bits + w - 1) // w, 1 << (w - 1)
    trows = (1 << w) + 1
    passes = -(-n_vec // tile)
    last = n_vec - (passes - 1) * tile
    S_max = max(slices, last_slices)
    x = Block("x", n_vec * cols, [v % mod for v in xs])
    xinv = Block("xinv", n_vec * cols, invert_batch(xs, mod)[0])      # all n_vec * cols elements, once, before the first pass
    out = Block("out", n_vec * rows)
    staged = transposed and tile < n_vec
    table = Block("table", tile * cols * trows)
    partial = Block("partial", S_max * tile * rows) if S_max > 1 else None
    stage = Block("stage", 2 * tile * cols) if staged else None
    for p in range(passes):
        v0, t = p * tile, last if p + 1 == passes else tile
        n_out = t * rows
        S = last_slices if p + 1 == passes else slices
        assert 1 <= S <= cols
        x_off = v0 if transposed else v0 * cols
        xt, xit, xt_off, xit_off = x, xinv, x_off, x_off
        dest = v0 if transposed else v0 * rows
        table.clear()                             # (the model's own: a row left by an earlier pass must not be read)
        if partial:
            partial.clear()
        if staged:
            stage.clear()
            s0 = 0
            s1 = tile * cols
            copy2d(stage, s0, t, x, x_off, n_vec, t, cols)
            copy2d(stage, s1, t, xinv, x_off, n_vec, t, cols)
            # [2][tile * cols]: the x^-1 half starts where a FULL tile of x would end, in the short last pass too
            assert stage.written() == list(range(t * cols)) + list(range(tile * cols, tile * cols + t * cols))
            xt, xit, xt_off, xit_off = stage, stage, s0, s1
        for item in range(2 * t * cols):          # matvec_signed_table_kernel: one group per (element, half)
            el, inv = item >> 1, item & 1
            tbl = el * trows
            base = (xit.rd(xit_off + el) if inv else xt.rd(xt_off + el))
            if not inv:
                table.wr(tbl, 1 % mod, once=True)
            tbl += h if inv else 0
            table.wr(tbl + 1, base, once=True)
            a = base
            for e in range(2, h + 1):
                a = a * base % mod
                table.wr(tbl + e, a, once=True)
        t_vec, t_col = (1, t) if transposed else (cols, 1)
        if S > 1:                                 # partial products [S][t][rows], transposed [S][rows][t]
            dst, base_at, o_slice, o_vec, o_row = partial, 0, n_out, (1 if transposed else rows), (t if transposed else 1)
        else:                                     # straight into the result batch
            dst, base_at, o_slice, o_vec, o_row = out, dest, 0, (1 if transposed else rows), (n_vec if transposed else 1)
        out_blocks = -(-n_out // ipw)
        for wave in range(S * out_blocks):        # matmul_signed_kernel
            s, blk = divmod(wave, out_blocks)
            lo, hi = s * cols // S, (s + 1) * cols // S
            assert lo < hi
            for grp in range(ipw):
                o = blk * ipw + grp
                live = o < n_out
                if not live:
                    o = n_out - 1                 # dead groups of the last wavefront walk the last output
                v, i = divmod(o, rows)
                assert v < t
                tvec, tcol = v * t_vec * trows, t_col * trows
                acc = table.rd(tvec + lo * tcol + kernel_row(wm[i][lo], w_words, e_bits, w, nwin - 1))
                for win in range(nwin - 1, -1, -1):
                    if win != nwin - 1:
                        for _ in range(w):
                            acc = acc * acc % mod
                    for j in range(lo + 1 if win == nwin - 1 else lo, hi):
                        acc = acc * table.rd(tvec + j * tcol + kernel_row(wm[i][j], w_words, e_bits, w, win)) % mod
                if live:
                    dst.wr(base_at + s * o_slice + v * o_vec + i * o_row, acc, once=True)
        cur = S                                   # the fold of pgpu_batch_ct_matmul
        while cur > 1:
            hh = (cur + 1) // 2
            to, to_at = (out, dest) if hh == 1 and not staged else (partial, 0)
            for k in range((cur - hh) * n_out):
                to.wr(to_at + k, partial.rd(k) * partial.rd(hh * n_out + k) % mod, once=to is out)
            cur = hh
        if S > 1 and staged:                      # [rows][t] back into [rows][n_vec]
            copy2d(out, dest, n_vec, partial, 0, t, t, rows, once=True)
    assert None not in out.v                      # ... and every slot was written (once: Block.wr)
    return out.v


def matmul_reference(xs, wm, mod, n_vec, transposed, e_bits):
    rows, cols = len(wm), len(xs) // n_vec
    out = [None] * (n_vec * rows)
    for v in range(n_vec):
        vec = [xs[j * n_vec + v] if transposed else xs[v * cols + j] for j in range(cols)]
        for i, y in enumerate(reference(vec, wm, mod, e_bits)):
            out[i * n_vec + v if transposed else v * rows + i] = y
    return out


def unit_values(rng, count, p, q):
    mod = (p * q) ** 2
    xs = ([1, mod - 1] + [rng.randrange(1, mod) for _ in range(count)])[:count]
    return [x if x % p and x % q else x + 1 for x in xs], mod


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("e_bits,w", [(13, 1), (13, 3), (13, 4), (13, 6), (32, 5), (70, 4)])
def test_matmul_signed_model_tiles_slices_windows(e_bits, w, transposed):
    """(5, 13, 33): tiles 1, 2 (a short last pass; transposed: staged, sliced, copied back) and 5, slices that do not divide
    33, e_bits no multiple of w, 70 bits in two words"""
    n_vec, rows, cols, g = 5, 13, 33, 4
    rng = random.Random(100 * e_bits + w)
    xs, mod = unit_values(rng, n_vec * cols, 1009, 1013)
    wm = stored_weights(rng, rows, cols, e_bits)
    want = matmul_reference(xs, wm, mod, n_vec, transposed, e_bits)
    assert all(want[v if transposed else v * rows] == 1 for v in range(n_vec))      # the zero row
    for tile in (1, 2, 5):
        for S in (1, 2, 5, 33):
            assert matmul_signed_model(xs, wm, mod, n_vec, transposed, e_bits, w, tile, S, S, g) == want, (tile, S)


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n_vec,rows,cols,tile,slices,last_slices,g", [
    (9, 6, 16, 8, 2, 4, 8),       # the shape of the GPU tests, fewer rows: one short pass of one vector on four slices
    (9, 3, 32, 8, 4, 8, 4),
    (5, 3, 32, 3, 5, 8, 8),       # the counts of 70 wavefronts per vector: the last pass fills more of the partial block, 8 * 2 > 5 * 3
    (3, 5, 7, 2, 2, 5, 4),        # ... and with a last pass of one vector: 5 * 1 > 2 * 2
    (3, 5, 7, 2, 1, 3, 2),        # no partial products in the full passes at all
    (7, 5, 9, 2, 3, 2, 8)])       # (and the other way round)
def test_matmul_signed_model_unequal_slices(n_vec, rows, cols, tile, slices, last_slices, g, transposed):
    """the short last pass on its own slice count inside blocks sized for a full tile; the counts are the plan's, passed in"""
    rng = random.Random(n_vec * 1000 + cols * 10 + last_slices)
    xs, mod = unit_values(rng, n_vec * cols, 251, 241)
    for e_bits, w in ((2, 1), (2, 2), (13, 4), (65, 3)):
        wm = stored_weights(rng, rows, cols, e_bits)
        want = matmul_reference(xs, wm, mod, n_vec, transposed, e_bits)
        assert matmul_signed_model(xs, wm, mod, n_vec, transposed, e_bits, w, tile, slices, last_slices, g) == want, (e_bits, w)


@pytest.mark.parametrize("g", [2, 4, 8])
@pytest.mark.parametrize("n_vec,rows", [(1, 33), (3, 11), (2, 8), (2, 4), (7, 5), (33, 1)])
def test_matmul_signed_model_outputs_around_a_wavefront(n_vec, rows, g):
    """33 outputs against the 32 / 16 / 8 groups of a wavefront, one column and nine; a tile of 2 keeps v = o / rows inside
    the tile for the clamped dead groups; weights one word wider than e_bits needs"""
    rng = random.Random(n_vec * 100 + rows + g)
    for cols in (1, 9):
        xs, mod = unit_values(rng, n_vec * cols, 1009, 1013)
        wm = [[v | (rng.getrandbits(64) << 64) for v in row] for row in stored_weights(rng, rows, cols, 32)]
        for transposed in (False, True):
            want = matmul_reference(xs, wm, mod, n_vec, transposed, 32)
            for tile in sorted({min(2, n_vec), n_vec}):
                S = min(cols, 3)
                assert matmul_signed_model(xs, wm, mod, n_vec, transposed, 32, 4, tile, S, S, g, w_words=2) == want, (cols, tile)


# ---- the plan queries ----
def _lib():
    from pailliercryptolib_amd import _capi
    return _capi.lib()


@pytest.fixture
def no_knobs(monkeypatch):
    for k in ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES", "PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES"):
        monkeypatch.delenv(k, raising=False)


def _mv_plan(L, signed, key_bits, rows, cols, e_bits):
    w, s, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    if signed:
        rc = L.pgpu_ct_matvec_signed_plan(key_bits, rows, cols, e_bits, ctypes.byref(w), ctypes.byref(s), ctypes.byref(tb), ctypes.byref(pr))
    else:
        rc = L.pgpu_ct_matvec_plan(key_bits, rows, cols, e_bits, ctypes.byref(w), ctypes.byref(s), ctypes.byref(tb))
    assert rc == 0
    return w.value, s.value, tb.value, pr.value


@pytest.mark.parametrize("key_bits", [1024, 2048, 3072])
@pytest.mark.parametrize("rows,cols,e_bits", [(1024, 1024, 32), (4096, 256, 32), (1, 1024, 32), (1, 1, 1), (5, 33, 64), (3, 1, 70)])
def test_matvec_signed_plan_contract(no_knobs, key_bits, rows, cols, e_bits):
    L = _lib()
    w, s, tb, pr = _mv_plan(L, True, key_bits, rows, cols, e_bits)
    uw, us, _, _ = _mv_plan(L, False, key_bits, rows, cols, e_bits)
    assert s == us                                                # the slices are the unsigned rule's
    assert tb == cols * ((1 << w) + 1) * ROW_BYTES[key_bits] and (tb <= CAP or w == 1)
    assert pr == planned_products(rows, cols, e_bits, w, s)
    fits = [v for v in WINDOWS if v == 1 or cols * ((1 << v) + 1) * ROW_BYTES[key_bits] <= CAP]
    assert pr == min(planned_products(rows, cols, e_bits, v, s) for v in fits)


def test_matvec_signed_plan_knobs_and_refusals(no_knobs, monkeypatch):
    L = _lib()
    monkeypatch.setenv("PGPU_MATVEC_WINDOW", "3")
    monkeypatch.setenv("PGPU_MATVEC_SLICES", "5")
    w, s, tb, pr = _mv_plan(L, True, 2048, 9, 40, 32)
    assert (w, s) == (3, 5) and tb == 40 * 9 * ROW_BYTES[2048] and pr == planned_products(9, 40, 32, 3, 5)
    monkeypatch.delenv("PGPU_MATVEC_WINDOW")
    monkeypatch.delenv("PGPU_MATVEC_SLICES")
    assert L.pgpu_ct_matvec_signed_plan(2048, 4, 4, 32, None, None, None, None) == 0       # every output is optional
    assert L.pgpu_ct_matvec_signed_plan(2048, 0, 4, 32, None, None, None, None) == -1
    assert L.pgpu_ct_matvec_signed_plan(2048, 4, 4, 0, None, None, None, None) == -1
    assert L.pgpu_ct_matvec_signed_plan(4096, 4, 4, 32, None, None, None, None) == -3      # no pair rows


@pytest.mark.parametrize("n_vec,rows,cols", [(1024, 16, 64), (64, 256, 256), (9, 5, 7), (1, 17, 9)])
def test_matmul_signed_plan_contract(no_knobs, n_vec, rows, cols):
    L = _lib()

    def plan(fn):
        w, s, t, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
        assert fn(2048, n_vec, rows, cols, 32, ctypes.byref(w), ctypes.byref(s), ctypes.byref(t), ctypes.byref(tb), ctypes.byref(pr)) == 0
        return w.value, s.value, t.value, tb.value, pr.value
    w, s, t, tb, pr = plan(L.pgpu_ct_matmul_signed_plan)
    uw, us, ut, utb, upr = plan(L.pgpu_ct_matmul_plan)
    assert tb == t * cols * ((1 << w) + 1) * ROW_BYTES[2048] <= CAP
    if (w, t) == (uw, ut):                                        # the same plan: the unsigned count plus the inversion
        assert s == us and pr == upr + 3 * (n_vec * cols - 1)
    else:                                                         # the longer table moved the tile or the window
        assert ut * cols * ((1 << uw) + 1) * ROW_BYTES[2048] > CAP and pr >= upr + 3 * (n_vec * cols - 1)
    if n_vec == 1:
        mw, ms, _, mpr = _mv_plan(L, True, 2048, rows, cols, 32)    # one vector: the signed matvec's plan
        assert (w, s, pr) == (mw, ms, mpr)


def test_header_and_binding_cover_the_calls():
    from pailliercryptolib_amd import _capi
    hdr = open(os.path.join(ROOT, "include", "pgpu.h")).read()
    for name in ("pgpu_batch_ct_matvec_signed", "pgpu_batch_ct_matmul_signed", "pgpu_ct_matvec_signed_plan", "pgpu_ct_matmul_signed_plan"):
        assert "int " + name + "(" in hdr and name in _capi.SYMBOLS


def test_no_signed_matvec_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = _lib()
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(1)
    assert L.pgpu_batch_ct_matvec_signed(fake, fake, fake, 1, 32, ctypes.byref(out)) == -4 and not out.value
    assert L.pgpu_batch_ct_matmul_signed(fake, fake, fake, 1, 1, 32, 0, ctypes.byref(out)) == -4 and not out.value
