"""The encrypted matrix product (pgpu_batch_ct_matmul; csrc/hensel_matmul.hpp) on the CPU.

1. An integer model of the exact schedule the call runs, in plain Python ints and with the ADDRESSES the host and the
   kernel form: the vectors walked in tiles (a short last pass included); per pass the window tables of the tile's elements
   (through the staging block where a pass of the transposed layout is not the whole of x); the outputs of a pass numbered
   flat, o = v * rows + i, across the groups of a wavefront -- a wavefront straddles vectors, the dead groups of the last
   one are clamped and do not store --; table rows and output rows through the two strides each; the matvec's
   multi-exponentiation per (output, column slice) with slices that need not divide cols and e_bits that need not be a
   multiple of w; the fold of the slices.  Checked against prod_j pow(x, w, n^2) for both layouts, every output row
   written exactly once, and its executed pair products against the count pgpu_ct_matmul_plan reports.
2. The contract of the host-side plan query pgpu_ct_matmul_plan (through ctypes; needs no device).
3. Without a device the call itself fails with PGPU_ERR_NO_DEVICE: there is no CPU fall-back."""
import ctypes
import random

import pytest

from test_matvec_model import GEOMETRY, K_SIMDS, digit

KNOBS = ("PGPU_MATMUL_WINDOW", "PGPU_MATMUL_TILE", "PGPU_MATMUL_SLICES")


def slices_rule(g, outputs, cols):
    """csrc/policy.cpp: the matvec's slice rule, for the outputs of one pass"""
    ipw = 64 // g
    waves = -(-outputs // ipw)
    return max(1, min(-(-K_SIMDS // waves), max(1, cols // 4), cols))


def reference(x, wm, mod, n_vec, transposed):
    rows, cols = len(wm), len(x) // n_vec
    out = [None] * (n_vec * rows)
    for v in range(n_vec):
        for i in range(rows):
            acc = 1 % mod
            for j in range(cols):
                acc = acc * pow(x[j * n_vec + v] if transposed else x[v * cols + j], wm[i][j], mod) % mod
            out[i * n_vec + v if transposed else v * rows + i] = acc
    return out


def model(x, wm, mod, n_vec, transposed, e_bits, w, tile, slices_of, g):
    """-> (the result batch, executed products: table, squarings, multiplications, fold; groups that ran a chain)"""
    rows, cols = len(wm), len(x) // n_vec
    ipw, nwin = 64 // g, (e_bits + w - 1) // w
    out = [None] * (n_vec * rows)
    n_table = n_sq = n_mul = n_fold = n_groups = 0
    staged = transposed and tile < n_vec
    for v0 in range(0, n_vec, tile):
        t = min(tile, n_vec - v0)
        S, n_out = slices_of(t), t * rows
        assert 1 <= S <= cols
        # the tile's elements as the table build sees them: a contiguous range
        if staged:
            xt = [x[j * n_vec + v0 + vl] for j in range(cols) for vl in range(t)]      # the 2-D copy: [cols][t]
        elif transposed:
            xt = x                                                                     # tile == n_vec: x itself
        else:
            xt = x[v0 * cols:(v0 + t) * cols]
        assert len(xt) == t * cols
        table = []
        for e in xt:                                  # matvec_table_kernel over t * cols elements
            row = [1 % mod, e % mod]
            for _ in range(2, 1 << w):
                row.append(row[-1] * e % mod)
                n_table += 1
            table.append(row[:1 << w])
        t_vec, t_col = (1, t) if transposed else (cols, 1)
        if S > 1:
            dst, o_slice, o_vec, o_row, base = [None] * (S * n_out), n_out, (1 if transposed else rows), (t if transposed else 1), 0
        else:
            dst, o_slice, o_vec, o_row = out, 0, (1 if transposed else rows), (n_vec if transposed else 1)
            base = v0 if transposed else v0 * rows
        out_blocks = -(-n_out // ipw)
        for wave in range(S * out_blocks):            # matmul_kernel: slice and column range are wavefront-uniform
            s, blk = divmod(wave, out_blocks)
            lo, hi = s * cols // S, (s + 1) * cols // S
            assert lo < hi
            for grp in range(ipw):
                o = blk * ipw + grp
                live = o < n_out
                if not live:
                    o = n_out - 1                     # dead groups of the last wavefront walk the last output
                v, i = divmod(o, rows)
                assert v < t
                acc = table[v * t_vec + lo * t_col][digit(wm[i][lo], nwin - 1, w, e_bits)]
                for win in range(nwin - 1, -1, -1):
                    if win != nwin - 1:
                        for _ in range(w):
                            acc = acc * acc % mod
                            n_sq += live
                    for j in range(lo + 1 if win == nwin - 1 else lo, hi):
                        acc = acc * table[v * t_vec + j * t_col][digit(wm[i][j], win, w, e_bits)] % mod
                        n_mul += live
                if live:
                    n_groups += 1
                    at = base + s * o_slice + v * o_vec + i * o_row
                    assert dst[at] is None            # every row is written once
                    dst[at] = acc
        if S > 1:
            cur = S                                   # the fold: slice h + k into slice k, over all outputs of the pass
            while cur > 1:
                h = (cur + 1) // 2
                for k in range((cur - h) * n_out):
                    dst[k] = dst[k] * dst[h * n_out + k] % mod
                    n_fold += 1
                cur = h
            for k in range(n_out):                    # the last product's store; staged: the 2-D copy [rows][t] -> pitch n_vec
                if transposed:
                    i, vl = divmod(k, t)
                    at = i * n_vec + v0 + vl
                else:
                    at = v0 * rows + k
                assert out[at] is None
                out[at] = dst[k]
    assert None not in out
    return out, (n_table, n_sq, n_mul, n_fold, n_groups)


def weights(rng, rows, cols, e_bits):
    wm = [[rng.getrandbits(e_bits) for _ in range(cols)] for _ in range(rows)]
    wm[0] = [0] * cols                                # an all-zero row: 1 for every vector
    if rows > 1:
        wm[1] = [(1 << e_bits) - 1] * cols
    return wm


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("n_vec,rows,cols", [(1, 1, 1), (1, 5, 33), (3, 5, 7), (7, 1, 9), (2, 17, 1), (5, 13, 33), (40, 3, 4)])
def test_model_flat_numbering_both_layouts(n_vec, rows, cols, transposed):
    rng = random.Random(n_vec * 10000 + rows * 100 + cols)
    mod = (65521 * 65537) ** 2
    x = [rng.randrange(1, mod) for _ in range(n_vec * cols)]
    for g in (2, 4, 8):                               # 32 / 16 / 8 groups per wavefront
        for e_bits, w in ((13, 4), (32, 5)):          # neither a multiple of w
            wm = weights(rng, rows, cols, e_bits)
            want = reference(x, wm, mod, n_vec, transposed)
            for tile in sorted({1, 2, n_vec}):
                if tile > n_vec:
                    continue
                got, _ = model(x, wm, mod, n_vec, transposed, e_bits, w, tile, lambda t: slices_rule(g, t * rows, cols), g)
                assert got == want, (g, e_bits, tile)
                if rows > 0:
                    assert all(want[(v if transposed else v * rows)] == 1 for v in range(n_vec))      # the zero row


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("w", [1, 4, 6])
@pytest.mark.parametrize("S", [1, 2, 5, 33])
def test_model_tiles_slices_windows(w, S, transposed):
    """(5, 13, 33): tiles 1, 2 (a short last pass) and 5, slices that do not divide 33, e_bits no multiple of w"""
    n_vec, rows, cols, g = 5, 13, 33, 4
    rng = random.Random(w * 100 + S)
    mod = (1009 * 1013) ** 2
    x = [rng.randrange(1, mod) for _ in range(n_vec * cols)]
    for e_bits in (13, 32):
        wm = weights(rng, rows, cols, e_bits)
        want = reference(x, wm, mod, n_vec, transposed)
        nwin = (e_bits + w - 1) // w
        for tile in (1, 2, 5):
            got, (nt, ns, nm, nf, ng) = model(x, wm, mod, n_vec, transposed, e_bits, w, tile, lambda t: S, g)
            assert got == want
            assert nt == n_vec * cols * ((1 << w) - 2)
            assert ng == n_vec * rows * S
            assert ns == ng * (nwin - 1) * w              # the top window needs no squarings
            assert nm == n_vec * rows * cols * nwin - ng  # the first position of every group is a load
            assert nf == n_vec * rows * (S - 1)


# ---- the plan query (host-only) ----
def _lib():
    from pailliercryptolib_amd import _capi, build
    build.build_pgpu()
    return _capi.lib()


def _plan(key_bits, n_vec, rows, cols, e_bits):
    L = _lib()
    w, s, t, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.pgpu_ct_matmul_plan(key_bits, n_vec, rows, cols, e_bits, ctypes.byref(w), ctypes.byref(s), ctypes.byref(t),
                               ctypes.byref(tb), ctypes.byref(pr))
    return rc, w.value, s.value, t.value, tb.value, pr.value


@pytest.fixture
def no_knobs(monkeypatch):
    for k in KNOBS + ("PGPU_MATVEC_WINDOW", "PGPU_MATVEC_SLICES"):
        monkeypatch.delenv(k, raising=False)
    return monkeypatch


@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("key_bits,n_vec,rows,cols,e_bits,forced", [
    (2048, 3, 5, 7, 13, None), (1024, 40, 3, 4, 32, None), (3072, 7, 1, 9, 32, None),
    (2048, 5, 13, 33, 32, (4, 2, 5)), (2048, 5, 13, 33, 13, (6, 2, 33)), (1024, 5, 13, 33, 13, (1, 5, 2))])
def test_model_products_equal_the_plan(no_knobs, key_bits, n_vec, rows, cols, e_bits, forced, transposed):
    """what the model executes, plus what the count includes and no group runs (the top window's squarings, the product
    the first position of a group saves), is the product count of the plan query"""
    g = GEOMETRY[key_bits][0]
    if forced:
        for k, v in zip(KNOBS, forced):
            no_knobs.setenv(k, str(v))
    rc, w, s, tile, tb, products = _plan(key_bits, n_vec, rows, cols, e_bits)
    assert rc == 0
    if forced:
        assert (w, tile, s) == forced
    slices_of = (lambda t: s) if forced else (lambda t: slices_rule(g, t * rows, cols))
    assert slices_of(tile) == s
    rng = random.Random(key_bits + n_vec)
    mod = (65521 * 65537) ** 2
    x = [rng.randrange(1, mod) for _ in range(n_vec * cols)]
    wm = weights(rng, rows, cols, e_bits)
    got, (nt, ns, nm, nf, ng) = model(x, wm, mod, n_vec, transposed, e_bits, w, tile, slices_of, g)
    assert got == reference(x, wm, mod, n_vec, transposed)
    nwin = (e_bits + w - 1) // w
    assert nt + ns + nm + nf + ng * (e_bits - (nwin - 1) * w) + ng == products


SHAPES = [(2048, 1, 1024, 1024, 32), (2048, 64, 256, 256, 32), (2048, 1024, 16, 64, 32), (2048, 4096, 64, 256, 32),
          (2048, 8, 8, 24, 32), (1024, 5, 13, 33, 13), (3072, 40, 3, 4, 32), (3072, 300, 7, 5000, 64), (2048, 3, 2, 1 << 20, 32)]


@pytest.mark.parametrize("key_bits,n_vec,rows,cols,e_bits", SHAPES)
def test_plan_contract(no_knobs, key_bits, n_vec, rows, cols, e_bits):
    rc, w, s, tile, tb, products = _plan(key_bits, n_vec, rows, cols, e_bits)
    assert rc == 0
    g, k = GEOMETRY[key_bits]
    row_bytes = 2 * g * k * 4
    assert 1 <= w <= 6 and 1 <= s <= cols and 1 <= tile <= n_vec
    assert tb == tile * cols * (1 << w) * row_bytes
    assert tb <= 256 << 20 or (tile == 1 and w == 1)          # the cap, but for one oversized vector
    assert s == slices_rule(g, tile * rows, cols)

    def call(v, t):
        def one(tv):
            S = slices_rule(g, tv * rows, cols)
            return tv * cols * ((1 << v) - 2) + tv * rows * S * e_bits + tv * rows * cols * -(-e_bits // v) + tv * rows * (S - 1)
        return (n_vec // t) * one(t) + (one(n_vec % t) if n_vec % t else 0)
    assert products == call(w, tile)
    # no other window at the tile its table allows (the largest, and a few below it) has fewer products
    for v in range(1, 7):
        t_hi = min(n_vec, (256 << 20) // (cols * (1 << v) * row_bytes))
        for t in range(t_hi, max(0, t_hi - 8), -1):
            assert call(v, t) >= products
    if n_vec == 1:
        from pailliercryptolib_amd import _capi
        mw, ms, mtb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
        assert _capi.lib().pgpu_ct_matvec_plan(key_bits, rows, cols, e_bits, ctypes.byref(mw), ctypes.byref(ms), ctypes.byref(mtb)) == 0
        assert (w, s, tile, tb) == (mw.value, ms.value, 1, mtb.value)


def test_plan_tiled_shape_beats_the_spmv_formulation(no_knobs):
    """4096 vectors x 256 columns -> 64 rows, 2048-bit key: tiled at a window above 1; the spmv plan of the same flat
    matrix is held at window 1 by the table over all columns"""
    n_vec, rows, cols = 4096, 64, 256
    rc, w, s, tile, tb, products = _plan(2048, n_vec, rows, cols, 32)
    assert rc == 0 and w > 1 and tile < n_vec and tb <= 256 << 20
    L = _lib()
    sw, sc, sl, stb, spr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    assert L.pgpu_ct_spmv_plan(2048, n_vec * rows, n_vec * cols, n_vec * rows * cols, cols, 32, ctypes.byref(sw), ctypes.byref(sc),
                               ctypes.byref(sl), ctypes.byref(stb), ctypes.byref(spr)) == 0
    assert sw.value == 1 and spr.value > 2 * products


def test_plan_forced_knobs_and_refusals(no_knobs):
    for k, v in zip(KNOBS, ("4", "2", "5")):
        no_knobs.setenv(k, v)
    assert _plan(2048, 5, 13, 33, 32)[:5] == (0, 4, 5, 2, 2 * 33 * 16 * 576)
    for k, v in zip(KNOBS, ("9", "77", "1000")):              # clamped: 1..6, 1..n_vec, 1..cols
        no_knobs.setenv(k, v)
    assert _plan(2048, 5, 13, 33, 32)[:4] == (0, 6, 33, 5)
    for k in KNOBS:
        no_knobs.delenv(k)
    L = _lib()
    assert _plan(4096, 4, 64, 64, 32)[0] == -3                # PGPU_ERR_UNSUPPORTED: no pair rows for this key class
    assert b"pair rows" in L.pgpu_last_error()
    for bad in ((0, 4, 4, 32), (4, 0, 4, 32), (4, 4, 0, 32), (4, 4, 4, 0)):
        assert _plan(2048, *bad)[0] == -1
    assert L.pgpu_ct_matmul_plan(2048, 4, 4, 4, 32, None, None, None, None, None) == 0      # every output is optional


def test_header_declares_the_call():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "pgpu.h")).read()
    assert "int pgpu_batch_ct_matmul(" in hdr and "int pgpu_ct_matmul_plan(" in hdr
    assert "#define PGPU_MATMUL_TRANSPOSED 1u" in hdr and "PGPU_KERNEL_MATMUL = 11" in hdr


def test_no_matmul_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    L = _lib()
    assert L.pgpu_device_count() == 0
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)                                 # never dereferenced: the readiness check comes first
    rc = L.pgpu_batch_ct_matmul(fake, fake, fake, 1, 1, 32, 0, ctypes.byref(out))
    assert rc == -4 and b"pgpu_init" in L.pgpu_last_error()       # PGPU_ERR_NO_DEVICE
    assert not out.value
