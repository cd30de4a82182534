"""The encrypted 2-D convolution (pgpu_batch_ct_conv2d; csrc/hensel_conv.hpp) on the CPU: an integer model of the exact
schedule the call runs, in plain Python ints and with the ADDRESSES the host and the kernel form.

The images walked in tiles of whole images (a short last pass included); per pass the window tables of the tile's
contiguous elements; the outputs of a pass numbered flat over [images of the tile][C_out][OH][OW] across the groups of a
wavefront -- a wavefront straddles rows, channels and images, the dead groups of the last one are clamped and do not
store --; the taps numbered flat, tap = (ci * kh + ky) * kw + kx, a slice a range [lo, hi) of them that need not divide
the taps, walked with (ci, ky, kx) carried along incrementally (one division at the slice's start); the table row of a tap
by arithmetic on the output position; a tap outside the image through digit 0 of a clamped, valid element; the fold of the
slices.  Checked against the direct definition with pow, every output row written exactly once, and its executed pair
products against the documented count.  Needs neither the library nor a device."""
import random

import pytest

from test_matvec_model import K_SIMDS, digit

# (n_img, C_in, H, W, C_out, kh, kw, sh, sw, ph, pw)
SHAPES = [
    (1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0),      # one element
    (1, 1, 1, 9, 1, 1, 3, 1, 1, 0, 1),      # conv1d; both edge outputs have a padded tap
    (2, 3, 5, 4, 2, 3, 2, 1, 1, 1, 0),      # everything non-square, padding on one axis only; 60 outputs
    (3, 1, 6, 6, 1, 2, 2, 2, 2, 0, 0),      # sum pooling
    (1, 1, 8, 7, 1, 3, 3, 2, 2, 0, 0),      # the floor in OH leaves the last image row unread
    (1, 2, 4, 5, 3, 4, 5, 1, 1, 0, 0),      # kernel equal to the image: a matvec
    (1, 3, 4, 5, 2, 1, 1, 1, 1, 0, 0),      # 1x1 kernel: a transposed matmul
    (1, 1, 3, 3, 1, 3, 3, 1, 1, 2, 2),      # maximal legal padding: corner outputs with one live tap out of nine
    (5, 2, 7, 3, 4, 3, 3, 2, 1, 1, 1),      # 240 outputs: more than one wavefront for every class
]
BIG = SHAPES[-1]


def out_size(shape):
    n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw = shape
    return (h + 2 * ph - kh) // sh + 1, (w + 2 * pw - kw) // sw + 1


def slices_rule(g, outputs, taps):
    """csrc/policy.cpp: the matvec's slice rule, for the outputs of one pass"""
    ipw = 64 // g
    waves = -(-outputs // ipw)
    return max(1, min(-(-K_SIMDS // waves), max(1, taps // 4), taps))


def reference(x, wt, mod, shape):
    """the definition: out[n][co][oy][ox] = prod x[n][ci][oy*sh + ky - ph][ox*sw + kx - pw]^w[co][ci][ky][kx], taps outside left out"""
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
                                    acc = acc * pow(x[((n * c_in + ci) * h + iy) * w + ix], wt[((co * c_in + ci) * kh + ky) * kw + kx], mod) % mod
                    out.append(acc)
    return out


def model(x, wt, mod, shape, e_bits, win_bits, tile, slices_of, g):
    """-> (the result batch, executed products: table, squarings, multiplications, fold; groups that ran a chain; padded
    positions multiplied by entry 0)"""
    n_img, c_in, h, w, c_out, kh, kw, sh, sw, ph, pw = shape
    oh, ow = out_size(shape)
    elems, n_o, taps = c_in * h * w, c_out * oh * ow, c_in * kh * kw
    ipw, nwin = 64 // g, (e_bits + win_bits - 1) // win_bits
    out = [None] * (n_img * n_o)
    n_table = n_sq = n_mul = n_fold = n_groups = n_pad = 0
    for i0 in range(0, n_img, tile):
        t = min(tile, n_img - i0)
        S, n_out = slices_of(t), t * n_o
        assert 1 <= S <= taps
        xt = x[i0 * elems:(i0 + t) * elems]               # the tile's images: a contiguous range of x
        table = []
        for e in xt:                                      # matvec_table_kernel over t * elems elements
            row = [1 % mod, e % mod]
            for _ in range(2, 1 << win_bits):
                row.append(row[-1] * e % mod)
                n_table += 1
            table.append(row[:1 << win_bits])
        dst = [None] * (S * n_out) if S > 1 else out
        base, o_slice = (0, n_out) if S > 1 else (i0 * n_o, 0)
        out_blocks = -(-n_out // ipw)
        for wave in range(S * out_blocks):                # conv_kernel: slice and tap range are wavefront-uniform
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
                    nonlocal n_pad
                    assert tap == (ci * kh + ky) * kw + kx and ci < c_in and ky < kh and kx < kw      # the incremental walk
                    iy, ix = y0 + ky, x0 + kx
                    inside = 0 <= iy < h and 0 <= ix < w
                    d = digit(wt[co * taps + tap], win, win_bits, e_bits) if inside else 0
                    n_pad += live and not inside
                    iy, ix = min(max(iy, 0), h - 1), min(max(ix, 0), w - 1)
                    row = table[((n * c_in + ci) * h + iy) * w + ix]     # clamped: always a row of the pass's table
                    assert inside or row[d] == 1 % mod
                    return row[d]
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
                    at = base + s * o_slice + o
                    assert dst[at] is None                # every row is written once
                    dst[at] = acc
        if S > 1:
            cur = S                                       # the fold: slice h + k into slice k, over all outputs of the pass
            while cur > 1:
                hh = (cur + 1) // 2
                for k in range((cur - hh) * n_out):
                    dst[k] = dst[k] * dst[hh * n_out + k] % mod
                    n_fold += 1
                cur = hh
            for k in range(n_out):
                assert out[i0 * n_o + k] is None
                out[i0 * n_o + k] = dst[k]
    assert None not in out
    return out, (n_table, n_sq, n_mul, n_fold, n_groups, n_pad)


def operands(rng, shape, mod, e_bits, pooling=False):
    n_img, c_in, h, w, c_out, kh, kw = shape[:7]
    x = [rng.randrange(2, mod) for _ in range(n_img * c_in * h * w)]
    n_w = c_out * c_in * kh * kw
    if pooling:
        return x, [1] * n_w
    wt = [rng.getrandbits(e_bits) for _ in range(n_w)]
    for k in range(0, n_w, 5):
        wt[k] = 0                                         # scattered zeros
    wt[n_w // 2] = (1 << e_bits) - 1
    return x, wt


@pytest.mark.parametrize("shape", SHAPES)
def test_model_equals_the_definition(shape):
    rng = random.Random(sum(v * 31 ** k for k, v in enumerate(shape)))
    mod = (65521 * 65537) ** 2
    n_img, taps = shape[0], shape[1] * shape[5] * shape[6]
    oh, ow = out_size(shape)
    n_o = shape[4] * oh * ow
    pooling = shape == SHAPES[3]
    for g in (2, 4, 8):                                   # 32 / 16 / 8 groups per wavefront
        for e_bits, win_bits in ((1, 1), (1, 4)) if pooling else ((13, 4), (32, 5)):
            x, wt = operands(rng, shape, mod, e_bits, pooling)
            want = reference(x, wt, mod, shape)
            assert len(want) == n_img * n_o
            for tile in sorted({1, 2, n_img}):
                if tile > n_img:
                    continue
                got, _ = model(x, wt, mod, shape, e_bits, win_bits, tile, lambda t: slices_rule(g, t * n_o, taps), g)
                assert got == want, (g, e_bits, tile)
                for S in {1, 2, taps}:
                    if S <= taps:
                        assert model(x, wt, mod, shape, e_bits, win_bits, tile, lambda t: S, g)[0] == want, (g, e_bits, tile, S)


def test_shapes_exercise_what_they_claim():
    """the flat numbering straddles and ends in dead groups; the edge cases of the padding"""
    s = SHAPES[2]
    oh, ow = out_size(s)
    assert s[0] * s[4] * oh * ow == 60 and 60 % 8 and 60 % 16 and 60 % 32      # dead groups in every class
    assert s[4] * oh * ow == 30                                                # a wavefront of 16 or 32 straddles images
    assert out_size(SHAPES[4]) == (3, 3) and (3 - 1) * 2 + 3 - 1 == 6 < 8 - 1       # the floor in OH: image row 7 is never read
    assert out_size(SHAPES[7]) == (5, 5)
    oh, ow = out_size(BIG)
    assert BIG[0] * BIG[4] * oh * ow == 240 and 240 > 2 * 32
    # sum pooling by the model: every output the product of its 2x2 block
    mod = (1009 * 1013) ** 2
    rng = random.Random(7)
    x, wt = operands(rng, SHAPES[3], mod, 1, pooling=True)
    got, _ = model(x, wt, mod, SHAPES[3], 1, 1, 3, lambda t: 1, 4)
    for n in range(3):
        for oy in range(3):
            for ox in range(3):
                blk = [x[(n * 6 + 2 * oy + dy) * 6 + 2 * ox + dx] for dy in (0, 1) for dx in (0, 1)]
                assert got[(n * 3 + oy) * 3 + ox] == blk[0] * blk[1] * blk[2] * blk[3] % mod
    # the corner outputs of maximal padding have one live tap out of nine
    x, wt = operands(rng, SHAPES[7], mod, 13)
    _, (_, _, _, _, ng, n_pad) = model(x, wt, mod, SHAPES[7], 13, 13, 1, lambda t: 1, 4)
    assert ng == 25 and n_pad == 25 * 9 - 81              # every (pixel, tap) pair is live in exactly one output
    # an all-zero filter gives the ciphertext 1
    assert set(reference(x, [0] * 9, mod, SHAPES[7])) == {1}
    assert set(model(x, [0] * 9, mod, SHAPES[7], 13, 4, 1, lambda t: 2, 4)[0]) == {1}


@pytest.mark.parametrize("win_bits", [1, 4, 6])
@pytest.mark.parametrize("S", [1, 2, 5, 18])
def test_model_tiles_slices_windows(win_bits, S):
    """the 240-output shape: tiles 1, 2 (a short last pass) and 5, slices that do not divide the 18 taps, e_bits no
    multiple of the window; the executed products against the documented count"""
    n_img, c_in, h, w, c_out, kh, kw = BIG[:7]
    oh, ow = out_size(BIG)
    elems, n_o, taps, g = c_in * h * w, c_out * oh * ow, c_in * kh * kw, 4
    rng = random.Random(win_bits * 100 + S)
    mod = (1009 * 1013) ** 2
    for e_bits in (13, 32):
        x, wt = operands(rng, BIG, mod, e_bits)
        want = reference(x, wt, mod, BIG)
        nwin = (e_bits + win_bits - 1) // win_bits
        for tile in (1, 2, 5):
            got, (nt, ns, nm, nf, ng, n_pad) = model(x, wt, mod, BIG, e_bits, win_bits, tile, lambda t: S, g)
            assert got == want
            assert nt == n_img * elems * ((1 << win_bits) - 2)
            assert ng == n_img * n_o * S
            assert ns == ng * (nwin - 1) * win_bits           # the top window needs no squarings
            assert nm == n_img * n_o * taps * nwin - ng       # padded taps are multiplied all the same; the first position is a load
            assert nf == n_img * n_o * (S - 1)
            assert n_pad > 0
            # ... which is the plan's count but for what the count includes and no group runs
            passes = [tile] * (n_img // tile) + ([n_img % tile] if n_img % tile else [])
            plan = sum(t * elems * ((1 << win_bits) - 2) + t * n_o * S * e_bits + t * n_o * taps * nwin + t * n_o * (S - 1) for t in passes)
            assert nt + ns + nm + nf + ng * (e_bits - (nwin - 1) * win_bits) + ng == plan
