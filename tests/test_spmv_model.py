"""The schedule of the encrypted sparse matrix-vector product (csrc/hensel_spmv.hpp: spmv_kernel, driven by the plan of
csrc/policy.cpp: spmv_plan) restated in plain integers modulo a small n^2: one chain per descriptor, 64/G chains per
wavefront, per window the wavefront's longest chain as the trip count (a chain past its own end multiplies by the row of
one, its column index and weight read at the clamped CSR position 0), w squarings before every window but the top one,
digits cut across 64-bit words with the top window masked below e_bits, idle chains of the last wavefront that do not
store, partial rows folded level by level by the segmented sum's schedule.  The plan is the real one -- printed by the
policy test binary, which is built from policy.cpp -- and the result is held against pow.  In the reference such a map is
composed from CipherText::operator* (ipcl/ciphertext.cpp:83-106) and operator+ (ciphertext.cpp:35-72)."""
import ctypes
import os
import random
import shutil
import subprocess

import pytest

from test_spmv_policy import build_policy_binary, clean_env

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NSQ = (1009 * 1013) ** 2
M64 = (1 << 64) - 1
pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")


@pytest.fixture(scope="module")
def planner(tmp_path_factory):
    exe = build_policy_binary(tmp_path_factory.mktemp("spmv_model"))

    def plan(row_ptr, chunk):
        text = f"{len(row_ptr) - 1} {chunk}\n" + " ".join(str(v) for v in row_ptr) + "\n"
        r = subprocess.run([exe, "plan"], input=text, capture_output=True, text=True, env=clean_env())
        assert r.returncode == 0, r.stdout
        lines = r.stdout.split("\n")
        if lines[0] == "refused":
            return None
        _, n_chains, partial_rows, _ = lines[0].split()
        chains = [tuple(int(v) for v in lines[1 + i].split()) for i in range(int(n_chains))]
        at = 1 + int(n_chains)
        levels = []
        for _ in range(int(lines[at].split()[1])):
            _, n_chunks, lv_partial = lines[at + 1].split()
            levels.append(([tuple(int(v) for v in lines[at + 2 + i].split()) for i in range(int(n_chunks))], int(lv_partial)))
            at += 1 + int(n_chunks)
        return chains, int(partial_rows), levels
    return plan


def digit(words, win, w, e_bits):
    """digit `win` of a weight held as 64-bit words, as spmv_kernel (and matvec_kernel) cut it"""
    nwin = -(-e_bits // w)
    bit = win * w
    word, sh = bit >> 6, bit & 63
    v = (words[word] >> sh) if word < len(words) else 0
    if sh + w > 64 and word + 1 < len(words):
        v |= (words[word + 1] << (64 - sh)) & M64
    if win == nwin - 1:
        v &= (1 << (e_bits - (nwin - 1) * w)) - 1
    return v & ((1 << w) - 1)


def run_spmv_kernel(table, col_idx, wwords, chains, out, partial, ipw, w, e_bits, stats):
    """spmv_kernel in integers"""
    n = len(chains)
    nwin = -(-e_bits // w)
    assert n >= 1
    for w0 in range(0, n, ipw):
        lanes = [min(w0 + g, n - 1) for g in range(ipw)]              # idle chains clamp to the last descriptor
        longest = max(1, max(chains[ci][1] for ci in lanes))          # at least one position per window
        for g, ci in enumerate(lanes):
            begin, length, dst, is_partial = chains[ci]

            def entry(t, win):
                pos = begin + t if t < length else 0                  # the clamped read: a valid CSR position
                col, d = col_idx[pos], digit(wwords[pos], win, w, e_bits)
                e = table[col][d]
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
                            stats["squarings"] += 1
                    acc = acc * entry(t, win) % NSQ
                    stats["products"] += 1
                    stats["padding"] += t >= length or w0 + g >= n
            if w0 + g < n:
                (partial if is_partial else out)[dst] = acc


def run_fold_kernel(src, chunks, out, partial, ipw):
    """segsum_kernel with the identity permutation, in integers (tests/test_segsum_model.py)"""
    n = len(chunks)
    for w0 in range(0, n, ipw):
        lanes = [min(w0 + g, n - 1) for g in range(ipw)]
        longest = max(chunks[ci][1] for ci in lanes)
        for g, ci in enumerate(lanes):
            begin, length, dst, is_partial = chunks[ci]
            row = lambda t: src[begin + t] if t < length else 1       # noqa: E731
            acc = row(0)
            for t in range(1, longest):
                acc = acc * row(t) % NSQ
            if w0 + g < n:
                (partial if is_partial else out)[dst] = acc


def to_words(v, words):
    return [(v >> (64 * i)) & M64 for i in range(words)]


def spmv_model(planner, xs, row_ptr, col_idx, weights, e_bits, w, chunk, ipw=16, words=None):
    rows = len(row_ptr) - 1
    words = words or -(-e_bits // 64)
    wwords = [to_words(v, words) for v in weights]
    table = [[pow(x, d, NSQ) for d in range(1 << w)] for x in xs]     # matvec_table_kernel: T[j][d] = x[j]^d
    chains, partial_rows, levels = planner(row_ptr, chunk)
    out, partial = [None] * rows, [None] * partial_rows
    stats = {"products": 0, "padding": 0, "squarings": 0, "levels": 1 + len(levels), "chains": len(chains)}
    run_spmv_kernel(table, col_idx, wwords, chains, out, partial, ipw, w, e_bits, stats)
    assert None not in partial
    for chunks, lv_partial in levels:
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
            acc = acc * pow(xs[col_idx[t]], weights[t] & ((1 << e_bits) - 1), NSQ) % NSQ
        out.append(acc)
    return out


def matrix(rng, lengths, cols):
    row_ptr = [0]
    for m in lengths:
        row_ptr.append(row_ptr[-1] + m)
    col_idx = [rng.randrange(cols) for _ in range(row_ptr[-1])]       # unsorted, duplicates allowed
    return row_ptr, col_idx


@pytest.mark.parametrize("e_bits", [1, 13, 64, 65])
@pytest.mark.parametrize("chunk", [1, 2, 3, 4, 64])
def test_schedule_equals_pow(planner, chunk, e_bits):
    """rows of 0, 1, chunk and chunk + 1 entries among others; e_bits not a multiple of w, a digit across a word boundary"""
    rng = random.Random(chunk * 100 + e_bits)
    cols = 11
    xs = [rng.randrange(1, NSQ) for _ in range(cols)]
    lengths = [0, 1, chunk, chunk + 1, 2, 0, 3, 7, 40, min(chunk * chunk + 1, 130), 1, 0]
    row_ptr, col_idx = matrix(rng, lengths, cols)
    weights = [rng.getrandbits(e_bits) for _ in col_idx]
    weights[0] = 0                                                    # a zero weight contributes 1
    weights[1] = (1 << e_bits) - 1
    want = direct(xs, row_ptr, col_idx, weights, e_bits)
    assert want[0] == want[5] == want[-1] == 1                        # empty rows: the ciphertext 1
    for w in (1, 2, 3, 4, 5, 6):
        for ipw in (8, 16, 32):                                       # 3072-, 2048- and 1024-bit key classes
            got, stats = spmv_model(planner, xs, row_ptr, col_idx, weights, e_bits, w, chunk, ipw)
            assert got == want, (w, ipw)
            fold_chunk, m, levels = max(2, chunk), -(-max(lengths) // chunk), 1
            if m > 1:
                levels += 1
                while m > fold_chunk:
                    m, levels = -(-m // fold_chunk), levels + 1
            assert stats["levels"] == levels
            assert stats["chains"] == sum(max(1, -(-m // chunk)) for m in lengths)


def test_duplicate_columns_contribute_twice(planner):
    xs = [5, 7, 11]
    row_ptr, col_idx, weights = [0, 3, 4], [1, 1, 1, 2], [3, 0, 9, 1]
    for chunk in (1, 2, 8):
        got, _ = spmv_model(planner, xs, row_ptr, col_idx, weights, 4, 2, chunk)
        assert got == [pow(7, 12, NSQ), 11]


def test_bits_above_e_bits_are_ignored(planner):
    rng = random.Random(3)
    xs = [rng.randrange(1, NSQ) for _ in range(6)]
    row_ptr, col_idx = matrix(rng, [3, 0, 5, 9], 6)
    for e_bits, words in ((13, 1), (64, 2), (65, 2), (1, 1)):
        weights = [rng.getrandbits(64 * words) | (1 << (64 * words - 1)) for _ in col_idx]     # bits set up to the top word
        want = direct(xs, row_ptr, col_idx, weights, e_bits)
        for w in (1, 4, 5, 6):
            got, _ = spmv_model(planner, xs, row_ptr, col_idx, weights, e_bits, w, 4, words=words)
            assert got == want, (e_bits, w)


def test_digits_cross_word_boundaries():
    e = (0x5 << 62) | 0x3                                             # bits 62..64 = 101 straddle the word boundary
    words = to_words(e, 2)
    assert digit(words, 12, 5, 65) == (e >> 60) & 31 == 20
    assert digit(words, 21, 3, 65) == (e >> 63) & 3 == 2              # the top window of 65 bits at w = 3: two bits
    assert digit(words, 10, 6, 65) == (e >> 60) & 31                  # ... at w = 6: five bits, across the boundary
    assert digit(to_words(M64, 1), 6, 5, 32) == 3                     # bits at and above e_bits are ignored


def test_padding_is_counted_and_a_wavefront_of_empty_rows_runs(planner):
    """ordered by length the chains of a wavefront differ by little; a wavefront whose chains are all empty walks one
    position per window and stores ones"""
    rng = random.Random(4)
    lengths = [0] * 40 + [5] * 20 + [1] * 30
    rng.shuffle(lengths)
    row_ptr, col_idx = matrix(rng, lengths, 9)
    xs = [rng.randrange(1, NSQ) for _ in range(9)]
    weights = [rng.getrandbits(13) for _ in col_idx]
    got, stats = spmv_model(planner, xs, row_ptr, col_idx, weights, 13, 4, 8, ipw=16)
    assert got == direct(xs, row_ptr, col_idx, weights, 13)
    useful = stats["products"] - stats["padding"]
    assert useful == 4 * sum(lengths) - sum(1 for m in lengths if m)  # nwin products per entry, the first of a chain saved
    assert stats["padding"] <= 0.5 * stats["products"], stats


# ---- the header and the plan query (host-only) ----
def test_header_carries_the_spmv_kind():
    hdr = open(os.path.join(ROOT, "include", "pgpu.h")).read()
    assert "PGPU_KERNEL_SPMV = 9" in hdr
    assert "PGPU_KERNEL_PACK = 8" in hdr
    assert "int pgpu_batch_ct_spmv(" in hdr and "int pgpu_ct_spmv_plan(" in hdr


def _plan(key_bits, rows, cols, nnz, longest, e_bits):
    from pailliercryptolib_amd import _capi, build
    build.build_pgpu()
    L = _capi.lib()
    w, c, lv, tb, pr = ctypes.c_int(), ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t(), ctypes.c_size_t()
    rc = L.pgpu_ct_spmv_plan(key_bits, rows, cols, nnz, longest, e_bits, ctypes.byref(w), ctypes.byref(c), ctypes.byref(lv),
                             ctypes.byref(tb), ctypes.byref(pr))
    return rc, w.value, c.value, lv.value, tb.value, pr.value


@pytest.fixture
def no_knobs(monkeypatch):
    monkeypatch.delenv("PGPU_SPMV_WINDOW", raising=False)
    monkeypatch.delenv("PGPU_SPMV_CHUNK", raising=False)
    return monkeypatch


def test_plan_call(no_knobs):
    # 65536 rows x 16 over 65536 columns, 32-bit weights, 2048-bit key: the table cap holds the window at 2
    rc, w, c, lv, tb, pr = _plan(2048, 65536, 65536, 1 << 20, 16, 32)
    assert (rc, w, c, lv) == (0, 2, 8, 2)
    assert tb == 65536 * 4 * 576
    chains = 65536 * 2                                                 # chunk 8 cuts every row of 16 in two
    assert pr == 65536 * 2 + chains * 32 + (1 << 20) * 16 + (chains - 65536)
    # one chain per row: the count is exact
    rc, w, c, lv, tb, pr = _plan(2048, 256, 256, 2048, 8, 32)
    assert (rc, c, lv) == (0, 4, 2) and 1 <= w <= 6 and tb == 256 * (1 << w) * 576
    rc, w, c, lv, tb, pr = _plan(1024, 100, 40, 300, 3, 1)
    assert (rc, w, c, lv, tb, pr) == (0, 1, 4, 1, 40 * 2 * 304, 100 * 1 + 300)
    no_knobs.setenv("PGPU_SPMV_WINDOW", "6")
    no_knobs.setenv("PGPU_SPMV_CHUNK", "2")
    assert _plan(3072, 9, 20, 60, 20, 13)[:4] == (0, 6, 2, 5)
    no_knobs.setenv("PGPU_SPMV_CHUNK", "1")
    assert _plan(3072, 9, 20, 60, 20, 13)[:4] == (0, 6, 1, 6)
    no_knobs.delenv("PGPU_SPMV_WINDOW")
    no_knobs.delenv("PGPU_SPMV_CHUNK")
    from pailliercryptolib_amd import _capi
    L = _capi.lib()
    assert _plan(4096, 64, 64, 64, 1, 32)[0] == -3                     # PGPU_ERR_UNSUPPORTED: no pair rows for this key class
    assert b"pair rows" in L.pgpu_last_error()
    for bad in ((0, 4, 4, 4, 1, 32), (2048, 0, 4, 4, 1, 32), (2048, 4, 0, 4, 1, 32), (2048, 4, 4, 0, 1, 32),
                (2048, 4, 4, 4, 0, 32), (2048, 4, 4, 4, 5, 32), (2048, 4, 4, 4, 1, 0), (2048, 2, 4, 7, 3, 32),
                (2048, 1 << 31, 4, 1 << 31, 1, 32), (2048, 4, 4, 1 << 31, 1 << 30, 32)):
        assert _plan(*bad)[0] == -1, bad                               # PGPU_ERR_INVALID_PARAM
    assert L.pgpu_ct_spmv_plan(2048, 4, 4, 4, 1, 32, None, None, None, None, None) == 0      # every output is optional
