"""Integer model of the Karatsuba form of psb_montmul (csrc/hensel_ps_bal.hpp, KARA; CPU test, no GPU): the single product of
two independent operands split in the middle, x = x0 + x1 B^H, y = y0 + y1 B^H,
    x y = L + (L + Hh + M) B^H + Hh B^2H,   L = x0 y0,  Hh = x1 y1,  M = (x0 - x1)(y1 - y0),
3 H^2 limb products instead of 4 H^2.  The model follows the kernel column by column with EVERY accumulator reduced modulo
2^64 -- the chains of L_k and Hh_k from a zero addend, the joins, the M products onto the column accumulator -- and checks
the digits, the result limbs and every column value against the schoolbook model of tests/test_ps_balanced_model.py.  Where
the M products land before the join, partial sums really do leave the 64-bit range (18 products of 2^59 on the extreme
operands: asserted below), and the wraps cancel: the finished column is the schoolbook column, whose bound (PsbFits) is
unchanged.  In the order of the source (the join first) no partial sum wraps at all; both orders are modelled.  A whole pair squaring
(the b part in this form, QMODE 2, x = 2a) and a whole pair product (its first product, QMODE 1) are checked against pow."""
import random

import pytest

from test_ps_balanced_model import HALF, K, KEYS, LB, ColumnLog, R, Side, limbs, montmul_limbs, num, sext

H = K // 2
M64 = (1 << 64) - 1


def s64(v):
    v &= M64
    return v - (1 << 64) if v >> 63 else v


class Wraps:
    """did a partial sum, taken as an integer, leave the signed 64-bit range?"""

    def __init__(self):
        self.count = 0
        self.top = 0

    def see(self, true_value):
        self.top = max(self.top, abs(true_value))
        if not -(1 << 63) <= true_value < (1 << 63):
            self.count += 1


def schoolbook_columns(x, y, n, q, qin=None):
    """the value of every column of psb_montmul's schoolbook form after its operand products (and the digit handed in),
    on unbounded integers, from the digits q the schoolbook model found"""
    cols, carry = [], 0
    for col in range(2 * K):
        lo, hi = (0, col) if col < K else (col - K + 1, K)
        v = carry + sum(q[i] * n[col - i] for i in range(lo, hi))
        lo, hi = (0, col + 1) if col < K else (col - K + 1, K)
        v += sum(x[i] * y[col - i] for i in range(lo, hi))
        if col < K:
            if qin is not None:
                v += qin[col]
            cols.append(v)
            assert (v + q[col] * n[0]) % (1 << LB) == 0
            carry = (v + q[col] * n[0]) >> LB
        else:
            cols.append(v)
            carry = (v + HALF) >> LB
    return cols


def kara_montmul(x, y, n, n0inv, qin=None, wraps=None, m_first=False):
    """psb_montmul<K, LB, 1, false, QMODE, false, true> column by column, every register 64 bits wide:
    (r limbs, digits q, carry out, the column values as the signed 64-bit numbers the kernel holds).
    m_first: the M products land on the accumulator before the join L_k + Hh_k does (the source adds the join first; the
    additions commute modulo 2^64, and the compiler's scheduler is free to emit either order)"""
    wraps = wraps or Wraps()
    dx = [x[j] - x[H + j] for j in range(H)]
    dy = [y[H + j] - y[j] for j in range(H)]
    assert all(-(1 << 31) <= v < (1 << 31) for v in dx + dy)       # int32_t
    lo, hi = {}, {}
    q, r, cols = [], [], []
    acc = true = 0                                                    # acc: the register; true: the same sum unreduced
    for col in range(2 * K):
        a, b = (0, col) if col < K else (col - K + 1, K)
        for i in range(a, b):
            acc = (acc + q[i] * n[col - i]) & M64
            true += q[i] * n[col - i]
            wraps.see(true)
        if col <= 2 * H - 2:
            a, b = (0, col + 1) if col < H else (col - H + 1, H)
            s = 0
            for i in range(a, b):
                s = (s + x[i] * y[col - i]) & M64
            lo[col] = s
            acc = (acc + s) & M64
            true += s64(s)
            wraps.see(true)
        if H <= col <= 3 * H - 2:
            k = col - H
            a, b = (0, k + 1) if k < H else (k - H + 1, H)
            s = 0
            for i in range(a, b):
                s = (s + x[H + i] * y[H + k - i]) & M64
            hi[k] = s
            u = (lo.pop(k) + s) & M64
            assert s64(u) == lo_true(x, y, k) + hi_true(x, y, k)      # the join itself fits: 36 products of 2^57
            if not m_first:
                acc = (acc + u) & M64
                true += s64(u)
                wraps.see(true)
            for i in range(a, b):
                acc = (acc + dx[i] * dy[k - i]) & M64
                true += dx[i] * dy[k - i]
                wraps.see(true)
            if m_first:
                acc = (acc + u) & M64
                true += s64(u)
                wraps.see(true)
        if 2 * H <= col <= 4 * H - 2:
            acc = (acc + hi.pop(col - 2 * H)) & M64
            true += s64(hi_true(x, y, col - 2 * H))
            wraps.see(true)
        assert len(lo) <= H + 1 and len(hi) <= H + 1                  # the sums that wait: at most 19 + 17 at once
        assert s64(acc) == true, col                                  # the finished column never wraps
        v = s64(acc)
        if col < K:
            if qin is not None:
                v += qin[col]
            cols.append(v)
            d = sext((v & 0xFFFFFFFF) * n0inv)
            q.append(d)
            v += d * n[0]
            assert -(1 << 63) <= v < (1 << 63) and v % (1 << LB) == 0
            v >>= LB
        else:
            cols.append(v)
            r.append(sext(v))
            v = (v + HALF) >> LB
        acc, true = v & M64, v
    assert not lo and not hi
    return r, q, s64(acc), cols


def lo_true(x, y, k):
    return sum(x[i] * y[k - i] for i in range(max(0, k - H + 1), min(k, H - 1) + 1))


def hi_true(x, y, k):
    return sum(x[H + i] * y[H + k - i] for i in range(max(0, k - H + 1), min(k, H - 1) + 1))


def check_against_schoolbook(x, y, n, n0inv, qin=None, wraps=None):
    """both orders of the join and the M products against the schoolbook model; wraps = (join first, products first)"""
    log = ColumnLog()
    r0, q0, c0 = montmul_limbs(x, y, n, n0inv, qin=qin, log=log)
    want = schoolbook_columns(x, y, n, q0, qin=qin)
    assert all(-(1 << 63) <= v < (1 << 63) for v in want)
    for m_first in (False, True):
        r1, q1, c1, cols = kara_montmul(x, y, n, n0inv, qin=qin, wraps=wraps[m_first] if wraps else None, m_first=m_first)
        assert (r1, q1, c1) == (r0, q0, c0)
        assert cols == want
    return r1, q1


P = KEYS["worst1040"][0]
S = Side(P, 0, 0)
# the largest modulus limbs (odd n_0), as the adversarial test of the schoolbook model takes them
N_MAX = [HALF if i else HALF - 1 for i in range(K)]
N0_MAX = (-pow(N_MAX[0], -1, 1 << LB)) % (1 << LB)


def test_sums_that_wait_fit_their_registers():
    """L_k and Hh_k are chains of at most H products of |x| <= 2^LB, |y| <= 2^(LB-1): 18 * 2^57 < 2^63, and so is their sum"""
    assert 2 * H * (1 << (2 * LB - 1)) < 1 << 63
    assert K % 2 == 0 and 3 * H * H == 972 and K * K == 1296


@pytest.mark.parametrize("qmode", [1, 2])
def test_random_balanced_operands(qmode):
    rng = random.Random(17 + qmode)
    for _ in range(12):
        a, b = (rng.randrange(-P // 2, P // 2) for _ in range(2))
        al, bl = limbs(a), limbs(b)
        if qmode == 2:                                                # the squaring's b part: x = 2a, the digits of a*a handed in
            x = [2 * v for v in al]
            _, qd, _ = montmul_limbs(al, al, S.nl, S.n0inv)
            r, _ = check_against_schoolbook(x, bl, S.nl, S.n0inv, qin=qd)
            assert num(r) == S.pmul((a, b), (a, b))[1]
        else:
            r, q = check_against_schoolbook(al, bl, S.nl, S.n0inv)
            t, Q = S.redc(a * b)
            assert (num(r), num(q)) == (t, Q)
        # random limbs over the whole range, not the limbs of a number below p/2
        x = [rng.randrange(-2 * HALF, 2 * HALF + 1) for _ in range(K)]
        y = [rng.randrange(-HALF, HALF + 1) for _ in range(K)]
        qin = [rng.randrange(-HALF, HALF) for _ in range(K)] if qmode == 2 else None
        check_against_schoolbook(x, y, N_MAX, N0_MAX, qin=qin)


@pytest.mark.parametrize("name", ["iso", "2051", "worst1040", "c2048-tight", "c2048-heavy"])
def test_values_at_the_settled_size(name):
    """|value| near 0.54 p, both signs: where the window loop's values settle"""
    p = KEYS[name][0]
    side = Side(p, 0, 0)
    for sa in (1, -1):
        for sb in (1, -1):
            a, b = sa * (54 * p // 100), sb * (54 * p // 100 - 12345)
            al, bl = limbs(a), limbs(b)
            _, qd, _ = montmul_limbs(al, al, side.nl, side.n0inv)
            r, _ = check_against_schoolbook([2 * v for v in al], bl, side.nl, side.n0inv, qin=qd)
            assert num(r) == side.pmul((a, b), (a, b))[1]
            r, q = check_against_schoolbook(al, bl, side.nl, side.n0inv)
            assert (num(r), num(q)) == side.redc(a * b)


def test_extreme_limbs_wrap_and_the_wraps_cancel():
    """all limbs at +-2^28 (x = 2a: +-2^29) in every sign pattern of the four halves, flat and alternating inside a half.
    x0 = -x1 with y0 = -y1 makes every dx dy = 2^59 (or -2^59): 18 of them pass 2^63, so where the M products land before
    the join a partial sum wraps -- and the finished column is the schoolbook column all the same.  Where the join lands first
    (the order of the source) every partial sum is itself a sum of at most 2(k+1) + (17-k) <= 36 operand products of 2^57
    on the q*n terms, inside the schoolbook bound: nothing wraps at all"""
    wrapped = {}
    for xmag in (HALF, 2 * HALF):
        for sx0 in (1, -1):
            for sx1 in (1, -1):
                for sy0 in (1, -1):
                    for sy1 in (1, -1):
                        for alt in (False, True):
                            def half(s, mag):
                                return [s * mag * (-1 if alt and i & 1 else 1) for i in range(H)]
                            x = half(sx0, xmag) + half(sx1, xmag)
                            y = half(sy0, HALF) + half(sy1, HALF)
                            for qin in (None, [HALF - 1] * K, [-HALF] * K):
                                w = (Wraps(), Wraps())
                                check_against_schoolbook(x, y, N_MAX, N0_MAX, qin=qin, wraps=w)
                                assert w[0].count == 0 and w[0].top < 1 << 63
                                wrapped[xmag, sx0, sx1, sy0, sy1, alt, qin is None] = (w[1].count, w[1].top)
    # the patterns the split is weakest on: x0 = -x1, y0 = -y1, the doubled operand -- a partial sum really did wrap
    for key in ((2 * HALF, 1, -1, -1, 1, False, True), (2 * HALF, -1, 1, 1, -1, False, True),
                (2 * HALF, 1, -1, 1, -1, False, True), (2 * HALF, -1, 1, -1, 1, False, True)):
        count, top = wrapped[key]
        assert count > 0 and top >= 1 << 63, key
    # ... while equal halves have dx = dy = 0 and nothing to wrap
    assert wrapped[2 * HALF, 1, 1, 1, 1, False, True][0] == 0


def pairsqr(side, al, bl):
    """psb_pairsqr<K, LB, true, true> on limbs: t = sym(2a, a) with its digits (the same columns as a*a), b = (2a*b + q)
    reduced in the Karatsuba form, a = t"""
    t, qd, c = montmul_limbs(al, al, side.nl, side.n0inv)
    assert c == 0
    w, _, c, _ = kara_montmul([2 * v for v in al], bl, side.nl, side.n0inv, qin=qd)
    assert c == 0
    return t, w


def pairmul(side, al, bl, cl, dl):
    """psb_pairmul<K, LB, true>: t = a*c in the Karatsuba form with its digits, b = (a*d + b*c + q) reduced (two products,
    schoolbook)"""
    t, qd, c, _ = kara_montmul(al, cl, side.nl, side.n0inv)
    assert c == 0
    w, _, c = montmul_limbs(al, dl, side.nl, side.n0inv, x2=bl, y2=cl, qin=qd)
    assert c == 0
    return t, w


@pytest.mark.parametrize("name", ["iso", "2051", "worst1040", "c2048-tight", "c2048-heavy"])
def test_pair_squaring_and_pair_product_against_pow(name):
    p = KEYS[name][0]
    side = Side(p, 0, 0)
    rinv = pow(R, -1, side.psq)
    rng = random.Random(name)
    for _ in range(3):
        u, v = rng.randrange(side.psq), rng.randrange(side.psq)
        # u R and v R as pairs (a, b), z = a - p b, a in [0, p) (it counts exactly), b moved into (-p/2, p/2)
        x, y = (((a, b - p if b >= p // 2 else b)) for a, b in (side.pair(u * R), side.pair(v * R)))
        assert side.val(x) == u * R % side.psq and side.val(y) == v * R % side.psq
        xl = (limbs(x[0]), limbs(x[1]))
        # six squarings and a product, as a window runs them: (u^64 v) R
        for _ in range(6):
            xl = pairsqr(side, *xl)
            x = side.pmul(x, x)
            assert (num(xl[0]), num(xl[1])) == x
        xl = pairmul(side, xl[0], xl[1], limbs(y[0]), limbs(y[1]))
        x = side.pmul(x, y)
        assert (num(xl[0]), num(xl[1])) == x
        assert side.val(x) == pow(u, 64, side.psq) * v % side.psq * R % side.psq
        assert side.val(x) * rinv % side.psq == pow(u, 64, side.psq) * v % side.psq
