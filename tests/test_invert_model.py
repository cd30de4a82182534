"""The schedule of the batched inversion (pgpu_batch_ct_negate / pgpu_batch_ct_sub; csrc/hensel_invert.hpp, policy.cpp:
invert_plan) restated in Python integers, in the lazy Montgomery domain the kernels work in: rows hold X = c * R modulo N
as any representative below 2N, and the only operation is the pair product M(X, Y) = X * Y * R^-1.  Forward pass, recursion
over the chain totals, ONE inversion at the top, walk back -- with the running products written into the output buffer
itself, as the call does.  Held against pow(c, -1, N): exact inverses for every chunk and count, 3 (count - 1) products and
one inversion whatever the chunk, row t - 1 read before row t is overwritten, the fused subtract and the broadcast b."""
import random

import pytest

CHUNKS = [2, 3, 8]
COUNTS = [1, 2, 3, 7, 8, 9, 64, 65, 300]
P_, Q_ = (1 << 61) - 1, (1 << 89) - 1                 # two primes: n = p q, N = n^2, as for a (small) Paillier key
N = (P_ * Q_) ** 2
R = 1 << 320                                          # the radix of the rows: a power of two above 4N


class Domain:
    """the lazy Montgomery domain: counts products and inversions"""

    def __init__(self, seed):
        self.rng = random.Random(seed)
        self.products = self.inversions = 0
        self.rinv = pow(R, -1, N)
        self.one = R % N

    def lazy(self, v):                                # any representative below 2N is a valid operand
        return v % N + self.rng.randrange(2) * N

    def enter(self, c):
        return self.lazy(c * R)

    def leave(self, X):                               # the canonical plain value
        return X * self.rinv % N

    def M(self, X, Y):
        assert 0 <= X < 2 * N and 0 <= Y < 2 * N
        self.products += 1
        return self.lazy(X * Y * self.rinv)

    def host_inverse(self, X):
        self.inversions += 1
        return self.enter(pow(self.leave(X), -1, N))  # one row down as the plain value, its inverse up as a row


def chains(n, chunk):
    """invert_plan's chains of a level of n rows: (begin, len), consecutive, only the last one shorter"""
    if n <= chunk:
        return [(0, n)]
    return [(b, min(chunk, n - b)) for b in range(0, n, chunk)]


def invert_rows(D, X, chunk, mul=None):
    """out[i] = X[i]^-1 (mul: times mul[i]), all rows of the domain D; returns (out, levels)"""
    n = len(X)
    out = [None] * n
    state = ["empty"] * n                             # empty -> product -> inverse: what a row of out holds
    ch = chains(n, chunk)
    for b, ln in ch:                                  # forward: the running products of every chain, into out itself
        if n == 1:
            break                                     # (a chain of one entry has nothing to multiply: no launch)
        acc = X[b]
        out[b], state[b] = acc, "product"
        for t in range(1, ln):
            acc = D.M(acc, X[b + t])
            out[b + t], state[b + t] = acc, "product"
    levels = 1
    if len(ch) == 1:
        U = [D.host_inverse(out[n - 1] if n > 1 else X[0])]
    else:                                             # recursion over the totals, gathered side by side
        totals = [out[b + ln - 1] for b, ln in ch]
        U, deeper = invert_rows(D, totals, chunk)
        levels += deeper
    for j, (b, ln) in enumerate(ch):                  # walk back, every chain from the inverse of its total
        u = U[j]
        for t in range(ln - 1, 0, -1):
            assert state[b + t - 1] == "product"      # row t - 1 is read before row t is overwritten
            inv = D.M(out[b + t - 1], u)
            u = D.M(u, X[b + t])
            if mul is not None:
                inv = D.M(inv, mul[b + t])
            out[b + t], state[b + t] = inv, "inverse"
        if mul is not None:
            u = D.M(u, mul[b])
        out[b], state[b] = u, "inverse"
    assert all(s == "inverse" for s in state)
    return out, levels


def model_levels(chunk, count):
    levels = 1
    while count > chunk:
        count = -(-count // chunk)
        levels += 1
    return levels


def ciphertexts(rng, count):
    out = []
    while len(out) < count:
        c = rng.randrange(1, N)
        if c % P_ and c % Q_:
            out.append(c)
    return out


@pytest.mark.parametrize("chunk", CHUNKS)
def test_exact_inverses_and_the_product_count(chunk):
    rng = random.Random(chunk)
    for count in COUNTS:
        cs = ciphertexts(rng, count)
        D = Domain(count)
        X = [D.enter(c) for c in cs]
        out, levels = invert_rows(D, X, chunk)
        assert [D.leave(v) for v in out] == [pow(c, -1, N) for c in cs], (chunk, count)
        assert D.products == 3 * (count - 1) and D.inversions == 1, (chunk, count)
        assert levels == model_levels(chunk, count)
        assert all(v < 2 * N for v in out)


def test_counts_1_to_300_every_chunk():
    rng = random.Random(0)
    cs = ciphertexts(rng, 300)
    want = [pow(c, -1, N) for c in cs]
    for chunk in CHUNKS:
        for count in range(1, 301):
            D = Domain(count)
            out, _ = invert_rows(D, [D.enter(c) for c in cs[:count]], chunk)
            assert [D.leave(v) for v in out] == want[:count]
            assert (D.products, D.inversions) == (3 * (count - 1), 1)


@pytest.mark.parametrize("chunk", CHUNKS)
def test_fused_subtract(chunk):
    """the level-0 walk multiplies a[t] in before the store: count more products, no other launch"""
    rng = random.Random(100 + chunk)
    for count in COUNTS:
        a, b = ciphertexts(rng, count), ciphertexts(rng, count)
        D = Domain(count)
        out, _ = invert_rows(D, [D.enter(c) for c in b], chunk, mul=[D.enter(c) for c in a])
        assert [D.leave(v) for v in out] == [x * pow(y, -1, N) % N for x, y in zip(a, b)], (chunk, count)
        assert D.products == 3 * (count - 1) + count and D.inversions == 1


def test_broadcast_b():
    """b of one element: one inverse (no product at all), multiplied into every a[i]"""
    rng = random.Random(7)
    for count in COUNTS:
        a, (b,) = ciphertexts(rng, count), ciphertexts(rng, 1)
        D = Domain(count)
        (binv,), levels = invert_rows(D, [D.enter(b)], 8)
        assert D.products == 0 and D.inversions == 1 and levels == 1
        out = [D.M(D.enter(x), binv) for x in a]
        assert [D.leave(v) for v in out] == [x * pow(b, -1, N) % N for x in a]
        assert D.products == count


def test_edge_values_and_the_row_of_one():
    """1, N - 1, n + 1 and (n + 1)^(n - 1) in runs, at the start and the end of a chain; a group past its end multiplies by
    the row of one, which leaves U what it is"""
    n = P_ * Q_
    edge = [1, N - 1, n + 1, pow(n + 1, n - 1, N)]
    rng = random.Random(3)
    cs = edge + ciphertexts(rng, 5) + edge[::-1] + [1, 1, 1] + [N - 1] * 4
    for chunk in CHUNKS:
        D = Domain(chunk)
        out, _ = invert_rows(D, [D.enter(c) for c in cs], chunk)
        assert [D.leave(v) for v in out] == [pow(c, -1, N) for c in cs]
    D = Domain(1)
    u = D.enter(cs[5])
    assert D.leave(D.M(u, D.one)) == cs[5] and D.leave(D.M(D.one, u)) == cs[5]


def test_a_non_unit_has_no_inverse():
    """the grand total of a batch that holds 0, p or n is not a unit: the one inversion fails, after the forward pass"""
    rng = random.Random(5)
    for bad in (0, P_, P_ * Q_):
        cs = ciphertexts(rng, 9)
        cs[4] = bad
        D = Domain(9)
        with pytest.raises(ValueError):
            invert_rows(D, [D.enter(c) for c in cs], 3)
        assert D.products == 6 + 2 and D.inversions == 1          # both forward passes ran (9 rows, then 3 totals), no walk
