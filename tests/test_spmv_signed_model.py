"""The signed-weight encrypted sparse matrix-vector product (pgpu_batch_ct_spmv_signed; csrc/hensel_spmv_signed.hpp) on the
CPU: the schedule of tests/test_spmv_model.py restated for signed weights, in plain Python ints modulo a small n^2 and on
bounds-checked flat blocks.

One batched inversion of EVERY column of x, referenced or not; the table of 2^w + 1 rows per column over [x ; x^-1] (row 0 =
one, rows 1..h = x^1..x^h, rows h+1..2h = x^-1..x^-h); spmv_kernel's chains (the real plan, printed by the policy test
binary built from policy.cpp), the wavefront's longest chain as the trip count, the row of an entry from signed_digit_row
-- row d, or row h - d for a negative digit --; a position past a chain's end reading CSR position 0 and multiplying by the
row of one; the unchanged fold levels.  Held against Python's pow on signed exponents, and the executed products against
the documented count (csrc/policy.cpp: spmv_signed_products = the unsigned count + 3 (cols - 1)).  In the reference such a
map is composed from CipherText::operator* and operator+ term by term."""
import random
import shutil

import pytest

from test_signed_matvec_model import Block, invert_batch, kernel_row, signed_value, unit_values
from test_spmv_model import NSQ, matrix, planner, run_fold_kernel  # noqa: F401  (planner: a fixture)

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
P, Q = 1009, 1013


def run_spmv_signed_kernel(table, trows, col_idx, weights, w_words, chains, out, partial, ipw, w, e_bits, stats):
    """spmv_signed_kernel in integers; table: a Block of cols * trows rows"""
    n = len(chains)
    nwin, h = -(-e_bits // w), 1 << (w - 1)
    assert n >= 1
    for w0 in range(0, n, ipw):
        lanes = [min(w0 + g, n - 1) for g in range(ipw)]              # idle chains clamp to the last descriptor
        longest = max(1, max(chains[ci][1] for ci in lanes))          # at least one position per window
        for g, ci in enumerate(lanes):
            begin, length, dst, is_partial = chains[ci]
            live = w0 + g < n

            def entry(t, win):
                pos = begin + t if t < length else 0                  # the clamped read: a valid CSR position
                col, row = col_idx[pos], kernel_row(weights[pos], w_words, e_bits, w, win)
                assert 0 <= row < trows
                e = table.rd(col * trows + row)                       # addressed whatever the length says
                stats["negative rows"] += live and t < length and row > h
                return e if t < length else 1                         # a select between two rows, both addressed
            acc = None
            for win in range(nwin - 1, -1, -1):
                for t in range(longest):
                    if acc is None:
                        acc = entry(t, win)                           # the first position starts the accumulator
                        continue
                    if t == 0:
                        for _ in range(w):
                            acc = acc * acc % NSQ
                            stats["squarings"] += live
                    acc = acc * entry(t, win) % NSQ
                    stats["products"] += live
                    stats["padding"] += live and t >= length
            if live:
                (partial if is_partial else out)[dst] = acc


def spmv_signed_model(planner, xs, row_ptr, col_idx, weights, e_bits, w, chunk, ipw=16, w_words=None):
    """weights: stored values -> (the result, stats)"""
    rows, cols = len(row_ptr) - 1, len(xs)
    w_words = w_words or -(-e_bits // 64)
    h, trows = 1 << (w - 1), (1 << w) + 1
    xinv, n_inv = invert_batch(xs, NSQ)                               # every column, referenced or not
    stats = {"inversion": n_inv, "table": 0, "products": 0, "padding": 0, "squarings": 0, "negative rows": 0}
    table = Block("table", cols * trows)
    for item in range(2 * cols):                                      # matvec_signed_table_kernel over all columns
        el, half = item >> 1, item & 1
        base = xinv[el] if half else xs[el] % NSQ
        tbl = el * trows
        if not half:
            table.wr(tbl, 1, once=True)
        tbl += h if half else 0
        table.wr(tbl + 1, base, once=True)
        a = base
        for e in range(2, h + 1):
            a = a * base % NSQ
            stats["table"] += 1
            table.wr(tbl + e, a, once=True)
    assert table.written() == list(range(cols * trows))
    chains, partial_rows, levels = planner(row_ptr, chunk)
    out, partial = [None] * rows, [None] * partial_rows
    stats["levels"], stats["chains"] = 1 + len(levels), len(chains)
    run_spmv_signed_kernel(table, trows, col_idx, weights, w_words, chains, out, partial, ipw, w, e_bits, stats)
    assert None not in partial
    for chunks, lv_partial in levels:                                 # the unchanged fold levels
        nxt = [None] * lv_partial
        run_fold_kernel(partial, chunks, out, nxt, ipw)
        assert None not in nxt
        partial = nxt
    assert None not in out
    return out, stats


def direct(xs, row_ptr, col_idx, weights, e_bits):
    out = []
    for i in range(len(row_ptr) - 1):
        acc = 1
        for t in range(row_ptr[i], row_ptr[i + 1]):
            acc = acc * pow(xs[col_idx[t]], signed_value(weights[t], e_bits), NSQ) % NSQ
        out.append(acc)
    return out


def units(rng, cols):
    xs, mod = unit_values(rng, cols, P, Q)
    assert mod == NSQ
    return xs


@pytest.mark.parametrize("e_bits", [1, 2, 13, 32, 63, 64, 65, 70])
@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 64])
def test_schedule_equals_pow(planner, chunk, e_bits):
    """rows of 0, 1, chunk and chunk + 1 entries among others; e_bits not a multiple of w, a digit across a word boundary;
    the edge weights; the executed products against the documented count"""
    rng = random.Random(chunk * 100 + e_bits)
    cols = 11
    xs = units(rng, cols)
    lengths = [0, 1, chunk, chunk + 1, 2, 0, 3, 7, 40, min(chunk * chunk + 1, 130), 1, 0]
    row_ptr, col_idx = matrix(rng, lengths, cols)
    nnz, rows = row_ptr[-1], len(lengths)
    mask, top = (1 << e_bits) - 1, 1 << (e_bits - 1)
    weights = [rng.getrandbits(e_bits) for _ in col_idx]
    weights[:4] = [0, mask, top, top - 1]                             # 0, -1, -2^(e-1), 2^(e-1) - 1
    want = direct(xs, row_ptr, col_idx, weights, e_bits)
    assert want[0] == want[5] == want[-1] == 1                        # empty rows: the ciphertext 1
    for w in (1, 2, 3, 4, 5, 6):
        nwin = -(-e_bits // w)
        for ipw in (8, 16, 32):                                       # 3072-, 2048- and 1024-bit key classes
            got, st = spmv_signed_model(planner, xs, row_ptr, col_idx, weights, e_bits, w, chunk, ipw)
            assert got == want, (w, ipw)
            chains = sum(max(1, -(-m // chunk)) for m in lengths)
            assert st["chains"] == chains
            assert st["inversion"] == 3 * (cols - 1) and st["table"] == cols * ((1 << w) - 2)
            assert st["squarings"] == chains * (nwin - 1) * w         # the top window needs no squarings
            useful = st["products"] - st["padding"]
            assert useful == nnz * nwin - sum(-(-m // chunk) for m in lengths)    # the first position of a chain is a load
            assert st["negative rows"] > 0
            # ... within the documented count: table, e_bits squarings per chain, nwin products per entry, the fold, the inversion
            fold = chains - rows
            plan = cols * ((1 << w) - 2) + chains * e_bits + nnz * nwin + fold + 3 * (cols - 1)
            assert st["inversion"] + st["table"] + st["squarings"] + useful + fold <= plan


def test_opposite_weights_on_one_column_cancel(planner):
    """a column named twice contributes twice: with weights a and -a the ciphertext 1 exactly, in one chain or in two"""
    xs = units(random.Random(1), 3)
    row_ptr, col_idx = [0, 2, 5, 5], [1, 1, 2, 0, 2]
    for e_bits, a in ((13, 1234), (64, (1 << 63) - 1), (70, 1 << 68)):
        mask = (1 << e_bits) - 1
        weights = [a, -a & mask, -a & mask, 7, a]
        for chunk in (1, 2, 8):
            for w in (1, 4, 6):
                got, _ = spmv_signed_model(planner, xs, row_ptr, col_idx, weights, e_bits, w, chunk)
                assert got == [1, pow(xs[0], 7, NSQ), 1], (e_bits, chunk, w)


def test_bits_above_e_bits_are_ignored(planner):
    rng = random.Random(3)
    xs = units(rng, 6)
    row_ptr, col_idx = matrix(rng, [3, 0, 5, 9], 6)
    for e_bits, words in ((13, 1), (64, 2), (65, 2), (1, 1), (70, 2)):
        weights = [rng.getrandbits(64 * words) | (1 << (64 * words - 1)) for _ in col_idx]     # bits set up to the top word
        want = direct(xs, row_ptr, col_idx, weights, e_bits)
        for w in (1, 4, 5, 6):
            got, _ = spmv_signed_model(planner, xs, row_ptr, col_idx, weights, e_bits, w, 4, w_words=words)
            assert got == want, (e_bits, w)


def test_positions_past_a_chain_end_and_a_wavefront_of_empty_rows(planner):
    """every weight negative, CSR position 0 included: a position past a chain's end addresses a row of x^-1 there and is
    multiplied by one all the same; a wavefront whose chains are all empty walks one position per window and stores ones"""
    rng = random.Random(4)
    lengths = [0] * 40 + [5] * 20 + [1] * 30
    rng.shuffle(lengths)
    row_ptr, col_idx = matrix(rng, lengths, 9)
    xs = units(rng, 9)
    weights = [(-rng.randrange(1, 1 << 12)) & ((1 << 13) - 1) for _ in col_idx]
    got, st = spmv_signed_model(planner, xs, row_ptr, col_idx, weights, 13, 4, 8, ipw=16)
    assert got == direct(xs, row_ptr, col_idx, weights, 13)
    assert st["padding"] > 0
    useful = st["products"] - st["padding"]
    assert useful == 4 * sum(lengths) - sum(1 for m in lengths if m)  # nwin products per entry, the first of a chain saved
