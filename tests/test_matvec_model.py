"""The encrypted matrix-vector product (pgpu_batch_ct_matvec; csrc/hensel_matvec.hpp) on the CPU.

1. An integer model of the exact schedule the kernels run, in plain Python ints: window tables T[j][d] = x[j]^d shared by
   all rows; per (row, column slice) an interleaved fixed-window multi-exponentiation from the top window down -- digits
   cut out of 64-bit words as the kernel cuts them (across word boundaries, the top window masked to e_bits), the top window
   without squarings, zero digits as multiplications by T[j][0] = 1 -- and the fold of the slices' partial products.  It
   is checked against  prod_j pow(x_j, w_ij, n^2) mod n^2  and its executed pair products against the count the window
   rule minimises (csrc/policy.hpp).
2. The contract of the host-side plan query pgpu_ct_matvec_plan (through ctypes; needs no device).
3. Without a device the call itself fails with PGPU_ERR_NO_DEVICE: there is no CPU fall-back.

What it stands for in the reference: a linear map composed from CipherText::operator* (ipcl/ciphertext.cpp:83-106) and
operator+ (ciphertext.cpp:35-72), term by term."""
import ctypes
import json
import os
import random

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M64 = (1 << 64) - 1
K_SIMDS = 1024
GEOMETRY = {1024: (2, 19), 2048: (4, 18), 3072: (8, 14)}      # (lanes per group, limbs per lane) of the key classes


def digit(e, win, w, e_bits):
    """csrc/hensel_matvec.hpp: the `digit` closure of matvec_kernel"""
    nwords = (e_bits + 63) // 64
    words = [(e >> (64 * k)) & M64 for k in range(nwords)]
    nwin = (e_bits + w - 1) // w
    bit = win * w
    word, sh = bit >> 6, bit & 63
    v = words[word] >> sh if word < nwords else 0
    if sh + w > 64 and word + 1 < nwords:
        v |= (words[word + 1] << (64 - sh)) & M64
    if win == nwin - 1:
        v &= (1 << (e_bits - (nwin - 1) * w)) - 1
    return v & ((1 << w) - 1)


def model(xs, wm, mod, e_bits, w, slices):
    """-> (results, executed products: table, squarings, multiplications, fold)"""
    rows, cols = len(wm), len(xs)
    assert 1 <= slices <= cols
    nwin = (e_bits + w - 1) // w
    n_table = n_sq = n_mul = n_fold = 0
    table = []
    for x in xs:                                  # matvec_table_kernel
        t = [1 % mod, x % mod]
        for _ in range(2, 1 << w):
            t.append(t[-1] * x % mod)
            n_table += 1
        table.append(t[:1 << w])
    part = [[None] * rows for _ in range(slices)]
    for s in range(slices):                       # matvec_kernel: one group per (row, slice)
        lo, hi = s * cols // slices, (s + 1) * cols // slices
        assert lo < hi
        for i in range(rows):
            acc = table[lo][digit(wm[i][lo], nwin - 1, w, e_bits)]       # the first position is a load
            for win in range(nwin - 1, -1, -1):
                if win != nwin - 1:
                    for _ in range(w):
                        acc = acc * acc % mod
                        n_sq += 1
                for j in range(lo + 1 if win == nwin - 1 else lo, hi):
                    acc = acc * table[j][digit(wm[i][j], win, w, e_bits)] % mod   # (digit 0: times one, no branch)
                    n_mul += 1
            part[s][i] = acc
    cur = slices                                  # the fold: slice h + k into slice k, ceil(log2 S) passes
    while cur > 1:
        h = (cur + 1) // 2
        for k in range(cur - h):
            for i in range(rows):
                part[k][i] = part[k][i] * part[k + h][i] % mod
                n_fold += 1
        cur = h
    return part[0], (n_table, n_sq, n_mul, n_fold)


def reference(xs, wm, mod):
    out = []
    for row in wm:
        acc = 1 % mod
        for x, e in zip(xs, row):
            acc = acc * pow(x, e, mod) % mod
        out.append(acc)
    return out


def planned_products(rows, cols, e_bits, w, slices):
    """csrc/policy.cpp: matvec_products -- what the window rule minimises"""
    return cols * ((1 << w) - 2) + rows * slices * e_bits + rows * cols * ((e_bits + w - 1) // w) + rows * (slices - 1)


def weights(rng, rows, cols, e_bits):
    top = (1 << e_bits) - 1
    wm = [[rng.getrandbits(e_bits) for _ in range(cols)] for _ in range(rows)]
    wm[0] = [0] * cols                              # an all-zero row: the result is 1
    if rows > 1:
        wm[1] = [top] * cols
    if rows > 2:
        wm[2] = [v if j % 3 else 0 for j, v in enumerate(wm[2])]
    return wm


@pytest.mark.parametrize("e_bits", [1, 5, 31, 32, 64, 127])
@pytest.mark.parametrize("w", [1, 2, 3, 4, 5, 6])
def test_schedule_model_small_moduli(e_bits, w):
    rng = random.Random(1000 * e_bits + w)
    for cols in (1, 2, 7):
        p, q = rng.choice([(1009, 1013), (65521, 65537), (2147483647, 4294967291)])
        n = p * q
        mod = n * n
        rows = 4
        xs = ([1, mod - 1] + [rng.randrange(1, mod) for _ in range(cols)])[:cols]
        wm = weights(rng, rows, cols, e_bits)
        want = reference(xs, wm, mod)
        assert want[0] == 1
        for slices in sorted({1, 2, 3, cols}):
            if slices > cols:
                continue
            got, (nt, ns, nm, nf) = model(xs, wm, mod, e_bits, w, slices)
            assert got == want, (cols, slices)
            nwin = (e_bits + w - 1) // w
            assert nt == cols * ((1 << w) - 2)
            assert ns == rows * slices * (nwin - 1) * w          # the top window needs no squarings
            assert nm == rows * (cols * nwin - slices)           # the first position of every group is a load
            assert nf == rows * (slices - 1)
            assert nt + ns + nm + nf <= planned_products(rows, cols, e_bits, w, slices)


@pytest.mark.parametrize("e_bits,w,slices", [(1, 1, 1), (5, 3, 2), (32, 4, 3), (64, 6, 5), (127, 5, 1)])
def test_schedule_model_kat_key(e_bits, w, slices):
    k = json.load(open(os.path.join(ROOT, "tests", "golden", "iso_kat.json")))
    n = int(k["p"], 16) * int(k["q"], 16)
    mod = n * n
    rng = random.Random(e_bits)
    cols, rows = 5, 3
    xs = [rng.randrange(1, mod) for _ in range(cols)]
    wm = weights(rng, rows, cols, e_bits)
    got, _ = model(xs, wm, mod, e_bits, w, slices)
    assert got == reference(xs, wm, mod)


def test_digits_cross_word_boundaries():
    e = (0x5 << 62) | (1 << 127) | 0x3                      # bits 62..64 = 101 straddle the first word boundary
    assert digit(e, 12, 5, 128) == ((e >> 60) & 31)
    assert digit(e, 21, 3, 128) == ((e >> 63) & 7)
    assert digit(e, 25, 5, 128) == (e >> 125) & 7           # the top window: 3 bits
    assert digit((1 << 127) - 1, 21, 6, 127) == 1           # top window of a 127-bit exponent at w = 6: one bit
    assert digit(M64, 6, 5, 32) == 3                        # bits at and above e_bits are ignored


# ---- the plan query (host-only) ----
def _plan(key_bits, rows, cols, e_bits):
    from pailliercryptolib_amd import _capi, build
    build.build_pgpu()
    L = _capi.lib()
    w, s, tb = ctypes.c_int(), ctypes.c_int(), ctypes.c_size_t()
    rc = L.pgpu_ct_matvec_plan(key_bits, rows, cols, e_bits, ctypes.byref(w), ctypes.byref(s), ctypes.byref(tb))
    return rc, w.value, s.value, tb.value


@pytest.fixture
def no_knobs(monkeypatch):
    monkeypatch.delenv("PGPU_MATVEC_WINDOW", raising=False)
    monkeypatch.delenv("PGPU_MATVEC_SLICES", raising=False)
    return monkeypatch


SHAPES = [(2048, 1, 1024, 32), (2048, 64, 1024, 32), (2048, 1024, 1024, 32), (2048, 4096, 256, 32), (3072, 256, 512, 32),
          (2048, 256, 512, 64), (1024, 5, 33, 7), (2048, 1, 1, 1), (2048, 3, 1, 32), (2048, 1, 7, 127), (3072, 17, 64, 32)]


@pytest.mark.parametrize("key_bits,rows,cols,e_bits", SHAPES)
def test_plan_contract(no_knobs, key_bits, rows, cols, e_bits):
    rc, w, s, tb = _plan(key_bits, rows, cols, e_bits)
    assert rc == 0
    g, k = GEOMETRY[key_bits]
    row_bytes = 2 * g * k * 4
    assert 1 <= w <= 6 and 1 <= s <= cols
    assert tb == cols * (1 << w) * row_bytes
    # the window has the fewest products among the windows whose table fits the cap (256 MiB)
    fits = [v for v in range(1, 7) if v == 1 or cols * (1 << v) * row_bytes <= 256 << 20]
    assert planned_products(rows, cols, e_bits, w, s) == min(planned_products(rows, cols, e_bits, v, s) for v in fits)
    # the slices: never more than fill the chip, a slice keeps at least 4 columns (or S = 1)
    ipw = 64 // g
    row_waves = -(-rows // ipw)
    assert s == 1 or ((s - 1) * row_waves < K_SIMDS and cols // s >= 4)


@pytest.mark.parametrize("rows,cols", [(1024, 1024), (64, 1024)])
def test_plan_covers_every_simd(no_knobs, rows, cols):
    rc, w, s, _ = _plan(2048, rows, cols, 32)
    assert rc == 0
    assert rows * s * 4 // 64 >= K_SIMDS


def test_plan_forced_knobs_and_refusals(no_knobs):
    no_knobs.setenv("PGPU_MATVEC_WINDOW", "6")
    no_knobs.setenv("PGPU_MATVEC_SLICES", "5")
    assert _plan(2048, 64, 300, 32)[:3] == (0, 6, 5)
    no_knobs.setenv("PGPU_MATVEC_WINDOW", "1")
    no_knobs.setenv("PGPU_MATVEC_SLICES", "300")
    assert _plan(2048, 64, 300, 32) == (0, 1, 300, 300 * 2 * 576)
    no_knobs.setenv("PGPU_MATVEC_SLICES", "1000")           # clamped to cols
    assert _plan(2048, 64, 7, 32)[2] == 7
    no_knobs.delenv("PGPU_MATVEC_WINDOW")
    no_knobs.delenv("PGPU_MATVEC_SLICES")
    from pailliercryptolib_amd import _capi
    L = _capi.lib()
    assert _plan(4096, 64, 64, 32)[0] == -3                 # PGPU_ERR_UNSUPPORTED: no pair rows for this key class
    assert b"pair rows" in L.pgpu_last_error()
    assert _plan(2048, 0, 64, 32)[0] == -1 and _plan(2048, 4, 0, 32)[0] == -1 and _plan(2048, 4, 4, 0)[0] == -1
    assert L.pgpu_ct_matvec_plan(2048, 4, 4, 32, None, None, None) == 0      # every output is optional


def test_no_matvec_without_device():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from pailliercryptolib_amd import _capi, build
    build.build_pgpu()
    L = _capi.lib()
    assert L.pgpu_device_count() == 0
    out = ctypes.c_void_p()
    fake = ctypes.c_void_p(8)                               # never dereferenced: the readiness check comes first
    rc = L.pgpu_batch_ct_matvec(fake, fake, fake, 1, 32, ctypes.byref(out))
    assert rc == -4 and b"pgpu_init" in L.pgpu_last_error()      # PGPU_ERR_NO_DEVICE
    assert not out.value
