"""The schedule of the bucket-method encrypted matvec (csrc/hensel_bucket.hpp, capi_aggregate.inc:
pgpu_batch_ct_matvec_bucket) restated in plain integers and held against pow: digits of c bits, one bucket per digit and
(row, window), the buckets reduced to prod_d B_d^d by two running products in two levels, the windows combined by
Horner.  The products the model issues are counted and held against the plan's data-independent bounds (policy.hpp)."""
import random

import pytest

N = (1 << 127) - 1          # any modulus will do: the schedule is generic group arithmetic
MOD = N * N


class Counter:
    def __init__(self):
        self.n = 0

    def mul(self, a, b):
        self.n += 1
        return a * b % MOD


def default_block(c):
    return 1 << ((c + 1) // 2)


def digits(w, e_bits, c):
    """the W = ceil(e_bits / c) digits of w mod 2^e_bits, window 0 least significant; the top one may be narrower"""
    w &= (1 << e_bits) - 1
    return [(w >> (c * t)) & ((1 << c) - 1) for t in range((e_bits + c - 1) // c)]


def running(cnt, entries):
    """acc = prod_{i >= 1} entries[i], tot = prod_i entries[i]^i: the walk from the last entry down to entry 1, both
    started from the last entry (no product by a one)"""
    acc = tot = entries[-1]
    for i in range(len(entries) - 2, 0, -1):
        acc = cnt.mul(acc, entries[i])
        tot = cnt.mul(tot, acc)
    return acc, tot


def reduce_buckets(cnt, B, c, b):
    nb = (1 << c) // b
    if nb == 1:                                   # level 1 alone: tot is S
        return running(cnt, B)[1]
    if b == 1:                                    # level 2 alone, over the buckets themselves (U = B, every V is one)
        return running(cnt, B)[1]
    U, V = [], []
    for k in range(nb):
        acc, tot = running(cnt, B[k * b:(k + 1) * b])
        U.append(cnt.mul(acc, B[k * b]))
        V.append(tot)
    tot = running(cnt, U)[1]                      # prod_k U_k^k
    for _ in range(b.bit_length() - 1):
        tot = cnt.mul(tot, tot)
    for v in V:
        tot = cnt.mul(tot, v)
    return tot


def bucket_matvec(x, w, rows, e_bits, c, b, cnt):
    cols = len(x)
    W = (e_bits + c - 1) // c
    out = []
    for i in range(rows):
        S = []
        for t in range(W):
            B = [1] * (1 << c)                    # bucket 0 and every empty bucket: one
            filled = [False] * (1 << c)
            for j in range(cols):
                d = digits(w[i * cols + j], e_bits, c)[t]
                if d:
                    B[d] = cnt.mul(B[d], x[j]) if filled[d] else x[j]
                    filled[d] = True
            S.append(reduce_buckets(cnt, B, c, b))
        acc = S[W - 1]                            # Horner: pack_kernel with slot_bits = c
        for t in range(W - 2, -1, -1):
            for _ in range(c):
                acc = cnt.mul(acc, acc)
            acc = cnt.mul(acc, S[t])
        out.append(acc)
    return out


def issued_products(w, rows, cols, e_bits, c, b):
    """what the schedule issues for these weights, term by term: a bucket of m columns costs m - 1 products, a walk over
    len entries 2 (len - 2), level 1 one more per block for U, level 2 log2 b squarings and nb products by the V_k"""
    W, nb = (e_bits + c - 1) // c, (1 << c) // b
    nonzero = buckets = 0
    for i in range(rows):
        for t in range(W):
            ds = [digits(w[i * cols + j], e_bits, c)[t] for j in range(cols)]
            nonzero += sum(1 for d in ds if d)
            buckets += len({d for d in ds if d})
    if nb == 1 or b == 1:
        reduce_ = 2 * ((1 << c) - 2)
    else:
        reduce_ = nb * (2 * (b - 2) + 1) + 2 * (nb - 2) + (b.bit_length() - 1) + nb
    return (nonzero - buckets) + rows * W * reduce_ + rows * (W - 1) * (c + 1)


def plan_products(rows, cols, e_bits, c, b):
    W, nb = (e_bits + c - 1) // c, (1 << c) // b
    lb = b.bit_length() - 1
    return rows * W * cols + rows * W * nb * 2 * (b - 1) + rows * W * (2 * (nb - 1) + lb + nb) + rows * (W - 1) * (c + 1)


def edge_weights(e_bits, c, rng, count):
    """0, 2^e_bits - 1, 1, 2^(c t) at the window boundaries, a weight with bits set above e_bits, then random ones"""
    ws = [0, (1 << e_bits) - 1, 1]
    ws += [1 << (c * t) for t in range((e_bits + c - 1) // c)]
    ws += [(1 << (e_bits + 3)) | (1 << e_bits) | rng.getrandbits(e_bits)]
    while len(ws) < count:
        ws.append(rng.getrandbits(e_bits))
    return ws


def blocks(c):
    return sorted({default_block(c), 1, 2, 1 << c})


@pytest.mark.parametrize("c", range(1, 11))
def test_bucket_schedule_against_pow(c):
    rng = random.Random(1000 + c)
    for b in blocks(c):
        for e_bits in (1, 7, 13, 32, 64, 65):
            for cols in (1, 5, 67):
                rows = 2
                x = [rng.randrange(2, MOD) for _ in range(cols)]
                w = edge_weights(e_bits, c, rng, rows * cols)
                rng.shuffle(w)
                w = w[:rows * cols - 1] + [(1 << (e_bits + 3)) | rng.getrandbits(e_bits)]   # (one keeps bits above e_bits)
                cnt = Counter()
                got = bucket_matvec(x, w, rows, e_bits, c, b, cnt)
                for i in range(rows):
                    want = 1
                    for j in range(cols):
                        want = want * pow(x[j], w[i * cols + j] & ((1 << e_bits) - 1), MOD) % MOD
                    assert got[i] == want, (c, b, e_bits, cols, i)
                assert cnt.n == issued_products(w, rows, cols, e_bits, c, b), (c, b, e_bits, cols)
                assert cnt.n <= plan_products(rows, cols, e_bits, c, b), (c, b, e_bits, cols)


def test_bucket_all_zero_row_is_one():
    cnt = Counter()
    x = [3, 5, 7]
    assert bucket_matvec(x, [0, 0, 0, 1, 2, 3], 2, 13, 4, 4, cnt) == [1, 3 * 25 * 343 % MOD]


def test_bucket_edge_weights_every_window_boundary():
    rng = random.Random(7)
    for c, e_bits in ((4, 13), (3, 32), (8, 65), (10, 64)):
        ws = edge_weights(e_bits, c, rng, 0)
        x = [rng.randrange(2, MOD) for _ in ws]
        cnt = Counter()
        got = bucket_matvec(x, ws, 1, e_bits, c, default_block(c), cnt)[0]
        want = 1
        for xj, wj in zip(x, ws):
            want = want * pow(xj, wj & ((1 << e_bits) - 1), MOD) % MOD
        assert got == want


def test_running_products_identity():
    """tot of the walk is prod_i e_i^i and acc * e_0 is prod_i e_i, for every length the kernel meets (>= 2)"""
    rng = random.Random(3)
    for n in (2, 3, 4, 8, 32):
        e = [rng.randrange(2, MOD) for _ in range(n)]
        cnt = Counter()
        acc, tot = running(cnt, e)
        want_acc = want_tot = 1
        for i in range(1, n):
            want_acc = want_acc * e[i] % MOD
            want_tot = want_tot * pow(e[i], i, MOD) % MOD
        assert (acc, tot) == (want_acc, want_tot)
        assert cnt.n == 2 * (n - 2)
