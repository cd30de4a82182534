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
3. The contract of the host-side plan queries pgpu_ct_matvec_signed_plan / pgpu_ct_matmul_signed_plan (ctypes; no device)."""
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
