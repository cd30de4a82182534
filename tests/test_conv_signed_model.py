"""The signed-weight encrypted 2-D convolution (pgpu_batch_ct_conv2d_signed; csrc/hensel_conv_signed.hpp) on the CPU: the
schedule of tests/test_conv_model.py restated for signed filters, in plain Python ints on bounds-checked flat blocks, with
the ADDRESSES the host (csrc/capi_aggregate.inc) and the kernel form.

One batched inversion of ALL of x before the first pass; per pass the table of 2^w + 1 rows per element over the tile's
contiguous range of x and x^-1 (row 0 = one, rows 1..h = x^1..x^h, rows h+1..2h = x^-1..x^-h); the flat output numbering,
the wavefront-uniform tap slices and the incremental (ci, ky, kx) walk of conv_kernel; the row of a tap from
signed_digit_row -- row d, or row h - d for a negative digit --; a tap outside the image on row 0 of a clamped, valid
element whatever its weight's sign; the fold.  Checked against the direct definition with Python's pow on signed
exponents, every output row written exactly once, no row outside a block touched and none read before it was written, and
the executed pair products against the documented count (csrc/policy.cpp: conv_signed_plan = the unsigned count +
3 (elements - 1)).  Needs neither the library nor a device."""
import random

import pytest

from test_conv_model import BIG, SHAPES, out_size, slices_rule
from test_signed_matvec_model import Block, invert_batch, kernel_row, signed_value, unit_values


def reference(x, wt, mod, shape, e_bits):
    """the definition with signed exponents (wt: stored weights), taps outside the image left out"""
    n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw = shape
    oh, ow = out_size(shape)
    out = []
    for n in range(n_img):
        for co in range(c_out):
            for oy in range(oh):
                for ox in range(ow):
                    acc = 1 % mod
                    for ci in range(c_in):
                        for ky in range(kh):
                            for kx in range(kw):
                                iy, ix = oy * sh + ky - ph, ox * sw + kx - pw
                                if 0 <= iy < h and 0 <= ix < w:
                                    e = signed_value(wt[((co * c_in + ci) * kh + ky) * kw + kx], e_bits)
                                    acc = acc * pow(x[((n * c_in + ci) * h + iy) * w + ix], e, mod) % mod
                    out.append(acc)
    return out


def model(xs, wt, mod, shape, e_bits, win_bits, tile, slices_of, g, w_words=None):
    """-> (the result batch, executed products: inversion, table, squarings, multiplications, fold; groups that ran a chain;
    padded positions multiplied by row 0; positions that selected a row of x^-1)"""
    n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw = shape
    oh, ow = out_size(shape)
    elems, n_o, taps = c_in * h * w, c_out * oh * ow, c_in * kh * kw
    w_words = w_words or (e_bits + 63) // 64
    ipw, nwin, hh = 64 // g, (e_bits + win_bits - 1) // win_bits, 1 << (win_bits - 1)
    trows = (1 << win_bits) + 1
    passes = -(-n_img // tile)
    S_max = max(slices_of(tile), slices_of(n_img - (passes - 1) * tile))
    x = Block("x", n_img * elems, [v % mod for v in xs])
    inv, n_inv = invert_batch(xs, mod)                    # all n_img * elems elements, once, before the first pass
    xinv = Block("xinv", n_img * elems, inv)
    out = Block("out", n_img * n_o)
    table = Block("table", tile * elems * trows)
    partial = Block("partial", S_max * tile * n_o) if S_max > 1 else None
    n_table = n_sq = n_mul = n_fold = n_groups = n_pad = n_neg = 0
    for i0 in range(0, n_img, tile):
        t = min(tile, n_img - i0)
        S, n_out = slices_of(t), t * n_o
        assert 1 <= S <= taps
        table.clear()                                     # (the model's own: a row left by an earlier pass must not be read)
        if partial:
            partial.clear()
        for item in range(2 * t * elems):                 # matvec_signed_table_kernel over the tile's range of x and x^-1
            el, half = item >> 1, item & 1
            tbl = el * trows
            base = (xinv if half else x).rd(i0 * elems + el)
            if not half:
                table.wr(tbl, 1 % mod, once=True)
            tbl += hh if half else 0
            table.wr(tbl + 1, base, once=True)
            a = base
            for e in range(2, hh + 1):
                a = a * base % mod
                n_table += 1
                table.wr(tbl + e, a, once=True)
        dst, base_at, o_slice = (partial, 0, n_out) if S > 1 else (out, i0 * n_o, 0)
        out_blocks = -(-n_out // ipw)
        for wave in range(S * out_blocks):                # conv_signed_kernel: slice and tap range are wavefront-uniform
            s, blk = divmod(wave, out_blocks)
            lo, hi = s * taps // S, (s + 1) * taps // S
            assert lo < hi
            lo_pos = (lo // (kh * kw), lo % (kh * kw) // kw, lo % kw)      # the only divisions of the walk
            for grp in range(ipw):
                o = blk * ipw + grp
                live = o < n_out
                if not live:
                    o = n_out - 1                         # dead groups of the last wavefront walk the last output
                ox, oy = o % ow, o // ow % oh
                co, n = o // ow // oh % c_out, o // ow // oh // c_out
                assert n < t
                y0, x0 = oy * sh - ph, ox * sw - pw

                def entry(tap, ci, ky, kx, win):
                    nonlocal n_pad, n_neg
                    assert tap == (ci * kh + ky) * kw + kx and ci < c_in and ky < kh and kx < kw      # the incremental walk
                    iy, ix = y0 + ky, x0 + kx
                    inside = 0 <= iy < h and 0 <= ix < w
                    row = kernel_row(wt[co * taps + tap], w_words, e_bits, win_bits, win)   # cut whatever `inside` says
                    assert 0 <= row < trows
                    row = row if inside else 0            # row 0 for a padded tap, whatever its weight's sign
                    n_pad += live and not inside
                    n_neg += live and row > hh
                    iy, ix = min(max(iy, 0), h - 1), min(max(ix, 0), w - 1)
                    elem = ((n * c_in + ci) * h + iy) * w + ix       # clamped: always an element of the pass's table
                    v = table.rd(elem * trows + row)
                    assert inside or v == 1 % mod
                    return v
                acc = None
                for win in range(nwin - 1, -1, -1):
                    tap, (ci, ky, kx) = lo, lo_pos
                    while tap < hi:
                        if acc is None:
                            acc = entry(tap, ci, ky, kx, win)             # the first position is a load
                        else:
                            if tap == lo:
                                for _ in range(win_bits):
                                    acc = acc * acc % mod
                                    n_sq += live
                            acc = acc * entry(tap, ci, ky, kx, win) % mod
                            n_mul += live
                        tap += 1
                        kx += 1
                        if kx == kw:
                            kx, ky = 0, ky + 1
                            if ky == kh:
                                ky, ci = 0, ci + 1
                if live:
                    n_groups += 1
                    dst.wr(base_at + s * o_slice + o, acc, once=True)      # every row is written once
        cur = S                                           # the fold of pgpu_batch_ct_conv2d
        while cur > 1:
            h2 = (cur + 1) // 2
            to, to_at = (out, i0 * n_o) if h2 == 1 else (partial, 0)
            for k in range((cur - h2) * n_out):
                to.wr(to_at + k, partial.rd(k) * partial.rd(h2 * n_out + k) % mod, once=to is out)
                n_fold += 1
            cur = h2
    assert None not in out.v
    return out.v, (n_inv, n_table, n_sq, n_mul, n_fold, n_groups, n_pad, n_neg)


def operands(rng, shape, p, q, e_bits, room=0):
    """units modulo (p q)^2 and stored weights: random, with scattered zeros, the four edge values, `room` garbage bits above
    e_bits"""
    n_img, c_in, h, w, c_out, kh, kw = shape[:7]
    x, mod = unit_values(rng, n_img * c_in * h * w, p, q)
    n_w = c_out * c_in * kh * kw
    mask, top = (1 << e_bits) - 1, 1 << (e_bits - 1)
    wt = [rng.getrandbits(e_bits) for _ in range(n_w)]
    for k in range(0, n_w, 5):
        wt[k] = 0                                         # scattered zeros
    for k, v in enumerate((top, top - 1, mask, 0)):       # -2^(e-1), 2^(e-1) - 1, -1, 0
        wt[(n_w // 2 + k) % n_w] = v
    if room:
        wt = [v | (rng.getrandbits(room) << e_bits) for v in wt]
    return x, wt, mod


@pytest.mark.parametrize("shape", SHAPES)
def test_model_equals_the_definition(shape):
    rng = random.Random(sum(v * 37 ** k for k, v in enumerate(shape)))
    n_img, taps = shape[0], shape[1] * shape[5] * shape[6]
    oh, ow = out_size(shape)
    n_o = shape[4] * oh * ow
    for g in (2, 4, 8):                                   # 32 / 16 / 8 groups per wavefront
        # (the 240-output shape has test_model_tiles_slices_windows to itself: one width here)
        for e_bits, win_bits in ((13, 4),) if shape == BIG else ((1, 1), (2, 2), (13, 4), (32, 5)):
            x, wt, mod = operands(rng, shape, 65521, 65537, e_bits)
            want = reference(x, wt, mod, shape, e_bits)
            assert len(want) == n_img * n_o
            for tile in sorted({1, min(2, n_img), n_img}):
                got, _ = model(x, wt, mod, shape, e_bits, win_bits, tile, lambda t: slices_rule(g, t * n_o, taps), g)
                assert got == want, (g, e_bits, tile)
                for S in {1, 2, taps}:
                    if S <= taps:
                        assert model(x, wt, mod, shape, e_bits, win_bits, tile, lambda t: S, g)[0] == want, (g, e_bits, tile, S)


@pytest.mark.parametrize("win_bits", [1, 2, 3, 4, 5, 6])
@pytest.mark.parametrize("S", [1, 2, 5, 18])
def test_model_tiles_slices_windows(win_bits, S):
    """the 240-output shape: tiles 1, 2 (a short last pass) and 5, slices that do not divide the 18 taps, e_bits no
    multiple of the window; the executed products against the documented count"""
    n_img, c_in, h, w, c_out, kh, kw = BIG[:7]
    oh, ow = out_size(BIG)
    elems, n_o, taps, g = c_in * h * w, c_out * oh * ow, c_in * kh * kw, 4
    rng = random.Random(win_bits * 100 + S)
    for e_bits in (13, 32):
        x, wt, mod = operands(rng, BIG, 1009, 1013, e_bits)
        want = reference(x, wt, mod, BIG, e_bits)
        nwin = (e_bits + win_bits - 1) // win_bits
        for tile in (1, 2, 5):
            got, (ni, nt, ns, nm, nf, ng, n_pad, n_neg) = model(x, wt, mod, BIG, e_bits, win_bits, tile, lambda t: S, g)
            assert got == want
            assert ni == 3 * (n_img * elems - 1)              # ONE inversion over all of x, whatever the tile
            assert nt == n_img * elems * ((1 << win_bits) - 2)   # 2 (h - 1) per element: as many as the unsigned table
            assert ng == n_img * n_o * S
            assert ns == ng * (nwin - 1) * win_bits           # the top window needs no squarings
            assert nm == n_img * n_o * taps * nwin - ng       # padded taps are multiplied all the same; the first position is a load
            assert nf == n_img * n_o * (S - 1)
            assert n_pad > 0 and n_neg > 0
            # ... which is the plan's count but for what the count includes and no group runs
            passes = [tile] * (n_img // tile) + ([n_img % tile] if n_img % tile else [])
            plan = sum(t * elems * ((1 << win_bits) - 2) + t * n_o * S * e_bits + t * n_o * taps * nwin + t * n_o * (S - 1) for t in passes)
            assert ni + nt + ns + nm + nf + ng * (e_bits - (nwin - 1) * win_bits) + ng == plan + 3 * (n_img * elems - 1)


@pytest.mark.parametrize("e_bits", [1, 2, 13, 32, 63, 64, 65, 70])
def test_model_e_bits_edges_and_garbage(e_bits):
    """every e_bits of the GPU test (70: a window starting at bit 64), rows one word wider than e_bits needs with garbage in
    the stored bits above e_bits, the edge weights, a short last pass on more slices than the full passes"""
    shape, g = SHAPES[2], 4
    n_o, taps = shape[4] * out_size(shape)[0] * out_size(shape)[1], shape[1] * shape[5] * shape[6]
    rng = random.Random(e_bits)
    w_words = (e_bits + 63) // 64 + 1
    x, wt, mod = operands(rng, shape, 251, 241, e_bits, room=64 * w_words - e_bits)
    want = reference(x, wt, mod, shape, e_bits)
    for win_bits in (1, 3, 4, 6):
        assert model(x, wt, mod, shape, e_bits, win_bits, 2, lambda t: 2, g, w_words=w_words)[0] == want, win_bits
    # (3 images, tile 2: the last pass of one image on 5 slices fills more of the partial block than a full pass on 2)
    x, wt, mod = operands(rng, (3,) + shape[1:], 251, 241, e_bits)
    got, _ = model(x, wt, mod, (3,) + shape[1:], e_bits, 4, 2, lambda t: 2 if t == 2 else 5, g)
    assert got == reference(x, wt, mod, (3,) + shape[1:], e_bits)


def test_padded_taps_land_on_row_zero_whatever_the_sign():
    """maximal legal padding with every weight negative: the corner outputs have one live tap out of nine, the eight others
    multiply by row 0 of a clamped element although their digits select rows of x^-1"""
    shape, e_bits = SHAPES[7], 13
    rng = random.Random(3)
    x, _, mod = operands(rng, shape, 1009, 1013, e_bits)
    mask = (1 << e_bits) - 1
    for wt in ([-1 & mask] * 9, [(1 << (e_bits - 1))] * 9, [(-v - 1) & mask for v in range(9)]):
        for win_bits in (1, 4, 6):
            got, (_, _, _, _, _, ng, n_pad, n_neg) = model(x, wt, mod, shape, e_bits, win_bits, 1, lambda t: 1, 4)
            assert got == reference(x, wt, mod, shape, e_bits)
            assert ng == 25 and n_pad == (25 * 9 - 81) * ((e_bits + win_bits - 1) // win_bits) and n_neg > 0
    # weights w and -w on the same pixels cancel: a 1x1 filter pair (w, -w) over two equal channels gives the ciphertext 1
    xs, mod = unit_values(rng, 12, 1009, 1013)
    shape = (1, 2, 3, 4, 1, 1, 1, 1, 1, 0, 0)
    got, _ = model(xs + xs, [1234, -1234 & mask], mod, shape, e_bits, 4, 1, lambda t: 1, 4)
    assert set(got) == {1}
    # an all-zero filter gives the ciphertext 1
    assert set(model(x, [0] * 9, mod, SHAPES[7], e_bits, 4, 1, lambda t: 2, 4)[0]) == {1}
